"""The numpy oracle run beside the vectorised DQN loop (VecDQN): every transition the device records and every TD / successor-
feature target it builds, restated from oracle.env alone -- the junction of the env, record, replay and target kernels, which
every other test compares with the project's own device path.  Test infrastructure, not a test module: nothing here needs a GPU,
so tests/test_cpu_vec_dqn_oracle_refs.py checks the references on a hand-made trace and shows that the defective twins are
rejected, and tests/test_gpu_vec_dqn_oracle.py applies the same rule to the loop.

* OracleTrack: one OracleLockstep per env, advanced by the action the device took (read from its record row).
* reference_targets: the targets of train_policy_net (successor_dqn.py:178-213 of the reference, oracle/dqn.py:15-31) with the
  batched readings of VecDQN's docstring -- n-step returns, double Q-learning -- on oracle-built rows through a module forward.
* accept: the rule of module_conforms (tests/test_gpu_conv_conformance.py): |got - ref64| <= FACTOR |lib32 - ref64| + 32 u max |ref64|
  in max norms, lib32 the same formula through the float32 library forward.  The allowance never looks at the code under test.
* undecided: a bootstrapping transition whose two largest q' (of the selecting net) lie closer in float64 than FACTOR times the
  measured max |q32 - q64| of its rows.  Its sf target -- and under double Q-learning its q target, which is the target net's value
  at the selected row and no maximum -- may follow either of the two rows; the plain q target is checked as it is: max is
  1-Lipschitz, |max q32 - max q64| <= max |q32 - q64|.
"""
import math

import numpy as np
import torch

from oracle.env import OracleLockstep
from robotoddler.training import records as R

U32 = 2.0 ** -24
FACTOR = 4.0
UNDECIDED_CAP = 0.10           # at most this share of the bootstrapping transitions of a case
MIN_DECIDED = 30               # and at least this many decided ones


class StableLockstep(OracleLockstep):
    """OracleLockstep with the candidate mask narrowed to the stable placements (stable_actions_only: filter_actions and then
    is_action_stable_rbe per action); a state with valid but no stable candidate is a reset-only lock-step as well."""

    def __init__(self, gym, capacity=16):
        super().__init__(gym, capacity)
        self._narrow()

    def _narrow(self):
        c = self.cand
        stable = np.zeros(len(c["actions"]), dtype=bool)
        for a in np.flatnonzero(c["mask"]):
            stable[a] = bool(self.gym.is_action_stable(c["actions"][a]))
        c["mask"] = c["mask"] & stable
        self.needs_reset = not c["mask"].any()

    def lockstep(self, pick_valid_rank):
        out = super().lockstep(pick_valid_rank)
        self._narrow()
        out["no_actions"] = self.needs_reset
        return out


class OracleTrack:
    """``make_gym(targets, obstacles) -> OracleGym`` (both None: the fixed task).  ``task_of(e) -> (targets, obstacles or None)``
    for envs that own their task: read from the device env's env_targets[e] / env_obstacles[e] whenever env e starts an episode
    (the draw itself is covered by tests/task_draw.py and tests/obstacle_draw.py).
    steps: the valid transitions in ring order (lock-step major, env minor), each a dict built from the oracle alone;
    grid[t][e]: the index into steps of env e's transition of lock-step t, or None for a reset-only lock-step."""

    def __init__(self, make_gym, n_envs, stable_actions_only=False, task_of=None):
        self.make_gym, self.E, self.task_of = make_gym, int(n_envs), task_of
        self.lockstep_cls = StableLockstep if stable_actions_only else OracleLockstep
        self.oracles = [self._fresh(e) for e in range(self.E)]
        self.last_frozen = [None] * self.E
        self.steps, self.grid = [], []

    def _fresh(self, e):
        targets, obstacles = self.task_of(e) if self.task_of is not None else (None, None)
        return self.lockstep_cls(self.make_gym(targets, obstacles))

    # ---- which candidate did the device take
    @staticmethod
    def match(oracle, row):
        """The index of the ONE valid oracle candidate the record row names: target block / face, shape, face and the pose
        (float64, compared exactly as tests/test_gpu_env_parity.py compares poses)."""
        c = oracle.cand
        key = tuple(int(row[o]) for o in (R.O_ATB, R.O_ATF, R.O_ASHAPE, R.O_AFACE))
        pose = tuple(float(v) for v in row[R.O_APOSE:R.O_APOSE + 4])
        hits = [int(a) for a in np.flatnonzero(c["mask"])
                if tuple(c["actions"][a][:4]) == key and (*c["blocks"][a].pos, *c["blocks"][a].cs) == pose]
        assert len(hits) == 1, f"the recorded action {key} {pose} matches {len(hits)} valid oracle candidates"
        return hits[0]

    def advance(self, rec, valid):
        """After agent.act(): rec [E, >= RECORD_WIDTH] float64 and valid [E] as numpy arrays."""
        picks = []
        for e, o in enumerate(self.oracles):
            assert bool(valid[e]) == (not o.needs_reset), f"env {e}: valid {bool(valid[e])}, the oracle's valid_step {not o.needs_reset}"
            picks.append(None if o.needs_reset else self.match(o, rec[e]))
        return self._advance(picks)

    def advance_random(self, rng):
        """An oracle-only lock-step under a seeded uniform pick (the CPU proxy of the undecided counts)."""
        return self._advance([None if o.needs_reset else int(rng.choice(np.flatnonzero(o.cand["mask"]))) for o in self.oracles])

    def _advance(self, picks):
        t, row = len(self.grid), []
        for e, (o, a) in enumerate(zip(self.oracles, picks)):
            g = o.gym
            if a is None:
                o.lockstep(None)
                ended = True
                row.append(None)
            else:
                c = o.cand
                valid_idx = np.flatnonzero(c["mask"])
                rank = int(np.searchsorted(valid_idx, a))
                tr = dict(env=e, t=t, nb=len(g.blocks), shapes=[g.shapes.index(b.shape) for b in g.blocks],
                          poses=[(*b.pos, *b.cs) for b in g.blocks], state=c["state"], cand_rasters=c["rasters"][valid_idx], pick=rank,
                          action=c["actions"][a], action_pose=(*c["blocks"][a].pos, *c["blocks"][a].cs), action_raster=c["rasters"][a],
                          stable_s=True if not g.blocks else bool(self.last_frozen[e]), reward_map=g.reward_map,
                          obstacle_raster=g.obstacle_raster, targets=g.targets, obstacles=g.obstacles)
                out = o.lockstep(lambda nv: rank)
                assert out["action_index"] == a
                tr.update(reward=out["reward"], lin=np.float32(out["lin_reward"]), done=out["done"], no_actions=out["no_actions"],
                          stable_frozen=bool(out["stable_frozen"]), stable_unfrozen=bool(out["stable_unfrozen"]))
                if not (out["done"] or out["no_actions"]):                # the transition bootstraps: s' and its valid candidates
                    tr["next_state"] = o.cand["state"]
                    tr["next_rasters"] = o.cand["rasters"][np.flatnonzero(o.cand["mask"])]
                ended = out["done"]
                row.append(len(self.steps))
                self.steps.append(tr)
            self.last_frozen[e] = None if ended else self.steps[row[-1]]["stable_frozen"]
            if ended and self.task_of is not None:
                self.oracles[e] = self._fresh(e)                          # the env starts an episode on the task it drew
        self.grid.append(row)
        return row


def ring_rows(track, n_step):
    """The rows the loop pushes to its ring, in ring order: per lock-step and env the h-step row of the oldest start once the
    window holds n_step transitions, and of every pending start (oldest first) when the episode ends (done | no_actions).
    -> [dict(window=[indices into track.steps, start first], h)]; n_step = 1: one row per transition."""
    rows, pending = [], [[] for _ in range(track.E)]
    for row in track.grid:
        for e, i in enumerate(row):
            if i is None:
                continue
            win = pending[e]
            win.append(i)
            tr = track.steps[i]
            if tr["done"] or tr["no_actions"]:
                rows += [dict(window=win[p:], h=len(win) - p) for p in range(len(win))]
                pending[e] = []
            elif len(win) == n_step:
                rows.append(dict(window=list(win), h=n_step))
                del win[0]
    return rows


def fold_return(lins, gamma):
    """(G, bound): the float64 n-step return sum_k gamma^k lin_k and tests/nstep_ref.py's bound on a float64 fold of it."""
    terms = [float(gamma) ** k * float(l) for k, l in enumerate(lins)]
    return math.fsum(terms), 2 * len(terms) * 2.0 ** -53 * math.fsum(abs(t) for t in terms)


TWINS = ("done_without_no_actions", "bootstrap_kept_when_done", "gamma_h_minus_1", "binary_of_next_state", "double_q_policy_value",
         "action_of_last_step", "current_task_map", "candidate_dropped")


def _images(a, like):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device=like.device, dtype=like.dtype)


def candidate_inputs(state, rasters, stable, reward_map, obstacle_raster, like):
    """The five inputs of a Q-network for the candidate rows ``rasters`` [m, S, S] of one state (get_state_features /
    get_action_features / get_task_features, successor_dqn.py:47-94): binary = [stable, 0, 0, 0, 0, 0]."""
    m = len(rasters)
    img = lambda a: _images(a, like).reshape(1, 1, *a.shape[-2:]).expand(m, -1, -1, -1)
    binary = torch.zeros((m, 6), dtype=like.dtype, device=like.device)
    binary[:, 0] = float(stable)
    return img(state), binary, _images(rasters, like).unsqueeze(1), img(reward_map), img(obstacle_raster)


def padded_forward(net, inputs, multiple=64):
    """net(*inputs) with the rows padded to a multiple of ``multiple`` by copies of row 0 (sliced off again): a rollout meets dozens
    of candidate counts, and a convolution library tunes per input shape -- two or three shapes instead."""
    m = inputs[0].shape[0]
    pad = (-m) % multiple
    if pad:
        inputs = [torch.cat([t, t[:1].expand(pad, *t.shape[1:])]) for t in inputs]
    return tuple(None if o is None else o[:m] for o in net(*inputs))


def first_maximum(q, rasters):
    """(best, second, gap) of the q [m] of the candidate rows ``rasters`` [m, S, S]: the first maximum; the runner-up, the largest q
    among the rows whose raster differs from the best row's -- candidates that attach the same shape by another face can cover the
    same pixels, their inputs and outputs are then the same numbers and "either row" says nothing about them (the first of them
    wins, here and in every evaluation); the gap between the two (None, inf without a runner-up)."""
    best = int(torch.argmax(q))                                                # torch.argmax: the first maximum
    other = torch.as_tensor(~(rasters == rasters[best]).all(axis=(1, 2)))
    if not bool(other.any()):
        return best, None, math.inf
    rest = q.clone()
    rest[~other.to(rest.device)] = -math.inf
    second = int(torch.argmax(rest))
    return best, second, float(q[best] - q[second])


@torch.no_grad()
def state_q(tr, net, reward_map=None, next_state=False):
    """q of ``net`` (module forward) over the valid candidates of the state a transition started in, or of the state it led to."""
    like = next(net.parameters())
    state, rasters, stable = ((tr["next_state"], tr["next_rasters"], tr["stable_frozen"]) if next_state else
                              (tr["state"], tr["cand_rasters"], tr["stable_s"]))
    return padded_forward(net, candidate_inputs(state, rasters, stable, tr["reward_map"] if reward_map is None else reward_map,
                                               tr["obstacle_raster"], like))[0]


@torch.no_grad()
def reference_td_errors(track, net_policy, maps=None, gamma=0.95):
    """td_error of every transition as the rollout records it (successor_dqn.py:413-426): |q(s, a) - (reward + gamma max_a' q(s', a'))|
    with the policy net, the next value 0 when done or when s' has no valid candidate -> float64 [len(track.steps)]."""
    out = []
    for i, tr in enumerate(track.steps):
        m = None if maps is None else maps[i]
        q = state_q(tr, net_policy, m)[tr["pick"]]
        nxt = state_q(tr, net_policy, m, next_state=True).max() if "next_rasters" in tr else torch.zeros_like(q)
        out.append((q - (float(tr["reward"]) + gamma * nxt)).abs().double().cpu())
    return torch.stack(out)


@torch.no_grad()
def reference_targets(track, rows, net_target, net_policy, gamma, n_step, double_q, use_sf, maps=None, pick=None, twin=None):
    """The inputs and targets of the ring rows ``rows`` (ring_rows) from the oracle's transitions, through the plain module forward
    of ``net_target`` / ``net_policy`` -- the float64 twins for the reference, the float32 nets under all_predicates_off() for the
    library's figure; everything behind the forward is evaluated in the nets' dtype.
        q  = G + gamma^h max_a' q'(s', a'),     sf = sum_{k<h} gamma^k raster_k + gamma^h psi'_0(s', argmax),
    G the float64 fold of the window's linear rewards (rounded to the nets' dtype), the bootstrap 0 when done or when s' has no valid
    candidate, the first maximum on a tie; double_q: the row is the policy net's first maximum, its value and psi' the target net's.
    ``maps`` [len(rows), S, S]: the reward map fed for every row (default: the oracle's).  ``pick`` [(best, second)] per row: the
    rows to read psi' (double_q: and q') at, instead of this evaluation's own arg-max -- the library figure at the reference's rows.
    ``twin``: one of TWINS, a deliberately defective evaluation.
    -> dict of float64 CPU tensors q [n], sf / sf_second [n, px] (use_sf; sf_second: the same with the runner-up row), q_second [n],
    gap [n] (between the largest selecting q' and the largest of a row with another raster, inf without one), boot [n] bool, block / action [n, S, S], binary [n, 6],
    map [n, S, S], and lists best / second (row of s' or None) and qsel (the selecting q' of every row of s')."""
    assert twin is None or twin in TWINS
    like = next(net_target.parameters())
    t_ = lambda v: torch.tensor(v, dtype=like.dtype, device=like.device)
    out = {k: [] for k in ("q", "q_second", "sf", "sf_second", "gap", "boot", "block", "action", "binary", "map", "best", "second", "qsel")}
    latest = {tr["env"]: tr for tr in track.steps}                            # twin 7: the task the env holds now
    for i, row in enumerate(rows):
        win = [track.steps[j] for j in row["window"]]
        first, last, h = win[0], win[-1], len(win)
        assert h == row["h"] and 1 <= h <= n_step
        G = t_(fold_return([tr["lin"] for tr in win], gamma)[0])
        order = win[::-1] if twin == "action_of_last_step" else win
        reward_map = (latest[first["env"]]["reward_map"] if twin == "current_task_map" else
                      first["reward_map"] if maps is None else maps[i])
        disc = t_(1.0)
        S = torch.zeros(first["action_raster"].shape, dtype=like.dtype, device=like.device)
        for tr in order:                                                       # ascending k, as the kernel adds them
            S = S + disc * _images(tr["action_raster"], like)
            disc = disc * t_(gamma)                                            # gamma^h after the loop
        if twin == "gamma_h_minus_1":
            disc = disc / t_(gamma)
        boot = not (last["done"] or last["no_actions"])
        if twin == "done_without_no_actions":
            boot = not last["done"]
        if twin == "bootstrap_kept_when_done":
            boot = len(last.get("next_rasters", ())) > 0
        q, q2, sf, sf2, gap, best, second, qsel = G, G, S, S, math.inf, None, None, None
        rasters = last.get("next_rasters", np.zeros((0,) + first["action_raster"].shape, dtype=bool)) if boot else None
        if boot and twin == "candidate_dropped":
            rasters = rasters[:-1]
        if boot and len(rasters) == 0:
            q = q2 = G + disc * t_(-math.inf)                                  # (a maximum over nothing: only a twin gets here)
        elif boot:
            inputs = candidate_inputs(last["next_state"], rasters, last["stable_frozen"], reward_map, last["obstacle_raster"], like)
            qt, psi, _ = padded_forward(net_target, inputs)
            qsel = padded_forward(net_policy, inputs)[0] if double_q else qt
            if twin == "double_q_policy_value":
                qt, psi, _ = padded_forward(net_policy, inputs)
            best, second, gap = first_maximum(qsel, rasters)
            own = (best, second)
            if pick is not None and pick[i][0] is not None:
                best, second = pick[i]
            at2 = best if second is None else second
            q = G + disc * (qt[best] if double_q else qt[own[0]])              # plain: this evaluation's own maximum
            q2 = G + disc * (qt[at2] if double_q else qt[own[0]])
            if use_sf:
                sf, sf2 = S + disc * psi[best, 0], S + disc * psi[at2, 0]
        binary = torch.zeros(6, dtype=torch.float64)
        binary[0] = float(first["stable_frozen"] if twin == "binary_of_next_state" else first["stable_s"])
        start = last if twin == "action_of_last_step" else first
        for k, v in (("q", q), ("q_second", q2), ("sf", sf.reshape(-1)), ("sf_second", sf2.reshape(-1)), ("gap", t_(gap)), ("boot", boot),
                     ("block", first["state"]), ("action", start["action_raster"]), ("binary", binary), ("map", reward_map),
                     ("best", best), ("second", second), ("qsel", None if qsel is None else qsel.double().cpu())):
            out[k].append(v)
    for k in ("q", "q_second", "sf", "sf_second", "gap"):
        out[k] = torch.stack([v.double().cpu() for v in out[k]])
    for k in ("block", "action", "map"):
        out[k] = torch.as_tensor(np.stack(out[k]).astype(np.float64))
    out["binary"], out["boot"] = torch.stack(out["binary"]), torch.tensor(out["boot"])
    if not use_sf:
        out["sf"] = out["sf_second"] = None
    return out


def accept(got, ref64, lib32):
    """module_conforms' rule in max norms over the tensors handed in -> (ok, share of the allowance used)."""
    got, ref64, lib32 = (torch.as_tensor(t).double().cpu().reshape(-1) for t in (got, ref64, lib32))
    assert got.shape == ref64.shape == lib32.shape and got.numel() > 0
    same = (got == ref64)                                                      # (an infinite reference is met exactly or not at all)
    err = float(torch.where(same, torch.zeros_like(got), (got - ref64).abs()).nan_to_num(nan=math.inf).max())
    finite = torch.isfinite(ref64)
    e_lib = float((lib32 - ref64)[finite].abs().max()) if bool(finite.any()) else 0.0
    allowance = FACTOR * e_lib + 32 * U32 * (float(ref64[finite].abs().max()) if bool(finite.any()) else 0.0)
    return err <= allowance, err / max(allowance, 1e-300)


def undecided(ref, lib):
    """bool [n]: the bootstrapping rows with a runner-up whose float64 gap is below FACTOR x the measured max |q32 - q64| of the
    selecting q' of their rows."""
    out = torch.zeros(len(ref["best"]), dtype=torch.bool)
    for i, (q64, q32) in enumerate(zip(ref["qsel"], lib["qsel"])):
        if q64 is not None and ref["second"][i] is not None:
            out[i] = float(ref["gap"][i]) < FACTOR * float((q32 - q64).abs().max())
    return out


def check_cap(ref, und, name=""):
    boot = int(ref["boot"].sum())
    n_und = int(und.sum())
    assert n_und <= UNDECIDED_CAP * boot, f"{name}: {n_und} of {boot} bootstrapping transitions undecided"
    assert boot - n_und >= MIN_DECIDED, f"{name}: only {boot - n_und} decided bootstrapping transitions"
    return boot - n_und, n_und


def conforms(got, ref, lib, und, double_q=False):
    """got: dict(q, sf or None, block, action, binary) of the code under test against reference_targets' ref (float64 twins) and
    lib (float32 library, evaluated with pick = ref's rows).  Inputs exact; q and sf through accept over all rows that take the
    reference's first maximum, and row by row against either near-tied row where undecided.  -> (ok, worst share, what failed)."""
    worst, failed = 0.0, []
    for k in ("block", "action", "binary"):
        if got.get(k) is not None and not torch.equal(torch.as_tensor(got[k]).double().cpu().reshape(ref[k].shape), ref[k]):
            failed.append(k)
    either = und if double_q else torch.zeros_like(und)
    for k, second, loose in (("q", "q_second", either), ("sf", "sf_second", und)):
        if ref[k] is None or got.get(k) is None:
            continue
        g = torch.as_tensor(got[k]).double().cpu().reshape(ref[k].shape)
        firm = ~loose
        if bool(firm.any()):
            ok, share = accept(g[firm], ref[k][firm], lib[k][firm])
            worst = max(worst, share)
            if not ok:
                failed.append(k)
        for i in torch.nonzero(loose).reshape(-1).tolist():
            tries = [accept(g[i], ref[k][i], lib[k][i]), accept(g[i], ref[second][i], lib[second][i])]
            worst = max(worst, min(s for _, s in tries))
            if not any(ok for ok, _ in tries):
                failed.append(f"{k}[{i}] (undecided)")
    return not failed, worst, failed


# ---------------------------------------------------------------------------------------------------------------------------
# The cases of tests/test_gpu_vec_dqn_oracle.py, and their CPU proxy: an oracle-only rollout under a seeded uniform pick with the
# twins' CPU forward, which shows that the reference alone stays inside the undecided cap at these seeds.
# A rollout is as small as the junctions allow (E envs, max_steps = 4, 10 or 6 lock-steps): at most E x lock-steps transitions, of
# which an n-step row bootstraps only when its window ends before the episode does -- fewer than MIN_DECIDED in one rollout of
# cases b, c and d whatever the policy.  A case therefore pools the rollouts of its ``seeds``; cap and minimum hold for the pool.
MAX_STEPS, GAMMA = 4, 0.95          # (td_errors hard-codes 0.95 as successor_dqn.py:425 does: at this gamma both readings agree)
OBSTACLE_RANGE = ((-3.0, 3.0), (0.3, 2.5))
MLP_LOSS = "mse_q_values+mse_block_features"
CASES = dict(
    a=dict(task="tower2", E=6, locksteps=10, net="mlp", loss=MLP_LOSS, agent={}, seeds=(1,)),
    b=dict(task="hexbridge", E=4, locksteps=6, net="mlp", loss=MLP_LOSS, agent=dict(stable_actions_only=True), seeds=(1, 2)),
    c=dict(task="tower2", E=6, locksteps=10, net="mlp", loss=MLP_LOSS, agent=dict(n_step=3), seeds=(1, 2, 3, 4)),
    d=dict(task="tower2", E=6, locksteps=10, net="mlp", loss=MLP_LOSS, agent=dict(double_q=True, n_step=3), seeds=(1, 2, 3, 4)),
    e=dict(task="random", E=6, locksteps=10, net="mlp", loss=MLP_LOSS, agent=dict(per_env_tasks=True, per_env_obstacles=True), seeds=(1,)),
    f=dict(task="tower2", E=6, locksteps=10, net="conv", loss="mse_q_values", agent={}, seeds=(1,)),
)


def case_setup(task):
    """-> (shape names, oracle setup dict) of a case's task; 'random': RandomTargets(2) and one RandomObstacles box, per env."""
    from oracle.env import bridge_setup, horizontal_bridge_setup
    if task == "tower2":
        return ["trapezoid"], bridge_setup(num_stories=2)
    if task == "hexbridge":
        return ["hexagon"], horizontal_bridge_setup(num_obstacles=3, trapezoid=False, hexagon=True)
    assert task == "random"
    return ["trapezoid"], dict(bridge_setup(num_stories=2), obstacles=None, targets=None)


def gym_factory(task):
    from oracle.env import OracleGym
    _, setup = case_setup(task)

    def make_gym(targets, obstacles):
        return OracleGym(setup["shapes"], setup["obstacles"] if obstacles is None else obstacles,
                         setup["targets"] if targets is None else targets, max_steps=MAX_STEPS)
    return make_gym


def make_nets(kind, seed, device):
    """(policy net, target net) as the GPU tests build them: init_weights under the seed, the target net mul_(1.05) of the policy."""
    import copy
    from robotoddler.models.cv import ConvNet, SuccessorMLP
    from robotoddler.utils.utils import init_weights
    torch.manual_seed(seed)
    net = (SuccessorMLP(img_size=(64, 64), hidden_dims=[256, 128, 64, 128, 256]) if kind == "mlp" else ConvNet(img_size=(64, 64))).to(device)
    net.apply(init_weights)
    target = copy.deepcopy(net)
    with torch.no_grad():
        for p in target.parameters():
            p.mul_(1.05)
    return net, target


def proxy_counts(name, seed):
    """(bootstrapping, undecided) ring rows of case ``name`` at ``seed`` from the oracle and the twins' CPU forward alone."""
    import copy
    from obstacle_draw import draw_obstacles
    from task_draw import draw_targets
    cfg = CASES[name]
    episode = [0] * cfg["E"]

    def task_of(e):
        episode[e] += 1
        return draw_targets(seed, e, episode[e] - 1, 2), draw_obstacles(seed, e, episode[e] - 1, [OBSTACLE_RANGE])
    track = OracleTrack(gym_factory(cfg["task"]), cfg["E"], stable_actions_only=cfg["agent"].get("stable_actions_only", False),
                        task_of=task_of if cfg["task"] == "random" else None)
    rng = np.random.default_rng(seed)
    for _ in range(cfg["locksteps"]):
        track.advance_random(rng)
    n_step, double_q = cfg["agent"].get("n_step", 1), cfg["agent"].get("double_q", False)
    rows = ring_rows(track, n_step)
    pol, tgt = make_nets(cfg["net"], seed, "cpu")
    args = (GAMMA, n_step, double_q, "mse_block_features" in cfg["loss"])
    ref = reference_targets(track, rows, copy.deepcopy(tgt).double(), copy.deepcopy(pol).double(), *args)
    lib = reference_targets(track, rows, tgt, pol, *args, pick=list(zip(ref["best"], ref["second"])))
    return int(ref["boot"].sum()), int(undecided(ref, lib).sum())


if __name__ == "__main__":       # the CPU proxy counts of docs/MEASUREMENT_LOG.md (run with the repository root and the package on PYTHONPATH)
    import sys
    for name in (sys.argv[1:] or sorted(CASES)):
        counts = [proxy_counts(name, s) for s in CASES[name]["seeds"]]
        boot, und = sum(b for b, _ in counts), sum(u for _, u in counts)
        print(f"P case {name} seeds {CASES[name]['seeds']}: bootstrapping {boot} undecided {und} per seed {counts}")
