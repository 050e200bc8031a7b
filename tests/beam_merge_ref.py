"""The rule of bridges_beam_merge (include/bridges_hip.h) stated once in numpy, the probe tables the kernel is run on, and defective
twins every probe set must tell from the rule.

A *case* is a dict of numpy arrays as the entry point takes them: B, K, key_last (ints), n_blocks int32 [E], blk_shape int32 [E, K],
blk_pose float64 [E, K, 4], blk_occ uint8 [E, K], targets_left int32 [E], live uint8 [E], ret float64 [E]; E = G * B.
``reference(case)`` returns the three outputs.  Nothing here compares floats where the rule compares bits: a pose word is its 64-bit
pattern; only ``ret`` is a number (a binary64 ``>``, a NaN below every number)."""
import numpy as np

TWINS = ("slot_by_slot", "ignores_last", "ignores_occ", "ignores_targets_left", "ignores_multiplicity", "across_groups",
         "matches_dead", "keeps_lower_ret", "ties_to_higher_env")
OUTPUTS = ("rep", "live", "n_merged")


def tuples(case, e, twin=None):
    """The block tuples of env e in slot order: uint64 [nb, 6] = shape id (as u32), occupancy, the four pose bit patterns."""
    K = case["K"]
    nb = min(max(int(case["n_blocks"][e]), 0), K)
    t = np.zeros((nb, 6), dtype=np.uint64)
    t[:, 0] = case["blk_shape"][e, :nb].astype(np.int32).view(np.uint32)
    t[:, 1] = 0 if twin == "ignores_occ" else case["blk_occ"][e, :nb]
    t[:, 2:] = np.ascontiguousarray(case["blk_pose"][e, :nb]).view(np.uint64).reshape(nb, 4)
    return t


def key(case, e, twin=None):
    """The key of env e as bytes: two keys are equal word for word iff the bytes are."""
    t = tuples(case, e, twin)
    nb = len(t)
    last = t[nb - 1:nb] if (case["key_last"] and nb and twin != "ignores_last") else t[:0]
    if twin == "slot_by_slot":
        body = t
    else:
        body = t[np.lexsort(t.T[::-1])] if nb else t             # rows in lexicographic order of their six words
        if twin == "ignores_multiplicity":
            body = np.unique(body, axis=0)
    tl = 0 if twin == "ignores_targets_left" else int(case["targets_left"][e])
    head = np.array([nb, tl], dtype=np.int64)
    return head.tobytes() + b"|" + last.tobytes() + b"|" + body.tobytes()


def ranks_before(case, a, b, twin=None):
    """Env a comes before env b among the envs of one class: ret descending (NaN last), then env index ascending."""
    ra, rb = case["ret"][a], case["ret"][b]

    def above(x, y):
        if np.isnan(x):
            return False
        if np.isnan(y):
            return True
        return bool(x < y) if twin == "keeps_lower_ret" else bool(x > y)
    if above(ra, rb):
        return True
    if above(rb, ra):
        return False
    return a > b if twin == "ties_to_higher_env" else a < b


def reference(case, twin=None):
    B, live = case["B"], case["live"]
    E = len(case["n_blocks"])
    assert E % B == 0
    alive = [bool(live[e]) or twin == "matches_dead" for e in range(E)]
    keys = [key(case, e, twin) if alive[e] else None for e in range(E)]
    rep = np.arange(E, dtype=np.int32)
    for e in range(E):
        if not alive[e]:
            continue
        mates = range(E) if twin == "across_groups" else range(e // B * B, (e // B + 1) * B)
        for o in mates:
            if o != e and alive[o] and keys[o] == keys[e] and ranks_before(case, o, int(rep[e]), twin):
                rep[e] = o
    live_out = np.array([1 if live[e] and rep[e] == e else 0 for e in range(E)], dtype=np.uint8)
    closed = np.array([1 if live[e] and rep[e] != e else 0 for e in range(E)], dtype=np.int32)
    return dict(rep=rep, live=live_out, n_merged=closed.reshape(E // B, B).sum(axis=1).astype(np.int32))


def sentinels(E, B):
    """What the output arrays hold before a call in the tests: values no call writes."""
    return dict(rep=np.full(E, -7, np.int32), live=np.full(E, 9, np.uint8), n_merged=np.full(E // B, -7, np.int32))


def same(a, b):
    return all(a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes() for k in OUTPUTS)


def _case(B, K, envs, key_last=1):
    """envs: per env a dict(blocks=[(shape, occ, (x, z, cos, sin)), ...], tl=, live=, ret=[, nb=]); the slots past the blocks hold
    junk (they are no part of a key)."""
    E = len(envs)
    c = dict(B=B, K=K, key_last=key_last, n_blocks=np.zeros(E, np.int32), blk_shape=np.full((E, K), 77, np.int32),
             blk_pose=np.full((E, K, 4), -9.25), blk_occ=np.full((E, K), 0xEE, np.uint8), targets_left=np.zeros(E, np.int32),
             live=np.zeros(E, np.uint8), ret=np.zeros(E))
    for e, env in enumerate(envs):
        blocks = env.get("blocks", [])
        assert len(blocks) <= K
        c["n_blocks"][e] = env.get("nb", len(blocks))
        for i, (shape, occ, pose) in enumerate(blocks):
            c["blk_shape"][e, i], c["blk_occ"][e, i], c["blk_pose"][e, i] = shape, occ, pose
        c["blk_shape"][e, len(blocks):] += e                         # junk that differs from env to env
        c["targets_left"][e], c["live"][e], c["ret"][e] = env.get("tl", 3), env.get("live", 1), env.get("ret", 0.0)
    return c


# a few blocks to build tables from: (shape id, occupancy, pose)
A_ = (0, 0b0001, (0.5, 0.25, 1.0, 0.0))
B_ = (0, 0b0000, (-1.5, 0.25, 1.0, 0.0))
C_ = (1, 0b0010, (0.5, 0.75, 0.0, 1.0))
D_ = (1, 0b0000, (2.0, 0.25, 1.0, 0.0))


def probe_tables():
    """name -> case: every corner the rule names, small enough to read."""
    t = {}
    env = lambda blocks, **kw: dict(blocks=list(blocks), **kw)
    # the same three blocks in two orders that end with the same block: one class, the higher return represents it
    t["permuted"] = _case(2, 6, [env([A_, B_, C_], ret=1.0), env([B_, A_, C_], ret=2.0)])
    # one bit of one pose word differs (and -0.0 is not 0.0): no class
    a_ulp = (0, 0b0001, (np.nextafter(0.5, 1.0), 0.25, 1.0, 0.0))
    a_neg = (0, 0b0001, (0.5, 0.25, 1.0, -0.0))
    t["one_bit_of_pose"] = _case(4, 6, [env([A_, B_]), env([a_ulp, B_]), env([a_neg, B_]), env([A_, B_], ret=-1.0)])
    # the occupancy of one block differs
    t["occupancy"] = _case(2, 6, [env([A_, B_, C_]), env([B_, (0, 0b0011, A_[2]), C_])])
    # targets_left differs
    t["targets_left"] = _case(2, 6, [env([A_, B_, C_], tl=3), env([B_, A_, C_], tl=1)])
    # the same multiset, another last block: a class only without key_last
    for kl in (0, 1):
        t[f"last_block_key_last_{kl}"] = _case(2, 6, [env([A_, B_], ret=0.5), env([B_, A_], ret=1.5)], key_last=kl)
    # equal tuples inside an env count: {A, A, B} is not {A, B, B} (both end with B ... and with A below)
    t["multiplicity"] = _case(4, 6, [env([A_, A_, B_]), env([A_, B_, B_]), env([B_, A_, A_], ret=1.0), env([A_, B_, A_], ret=2.0)])
    # empty envs are one class (no last block to hold against each other); a full env: every slot counts
    t["nb_0"] = _case(4, 3, [env([], ret=0.0), env([], ret=1.0), env([A_]), env([], tl=2)])
    full_a, full_b = [A_, B_, C_, D_], [D_, B_, A_, C_]
    t["nb_K"] = _case(4, 4, [env(full_a), env([C_, B_, A_, D_], ret=1.0), env(full_b), env(full_b, nb=9, ret=-1.0)])   # (nb clamps to K)
    # a dead duplicate with the best return neither represents nor is closed
    t["dead_duplicate"] = _case(4, 6, [env([A_, B_, C_], ret=1.0), env([B_, A_, C_], ret=9.0, live=0), env([B_, A_, C_], ret=0.5),
                                       env([A_], live=0)])
    # equal states in different groups
    t["other_group"] = _case(2, 6, [env([A_, B_, C_], ret=1.0), env([D_]), env([B_, A_, C_], ret=2.0), env([D_], live=0)])
    # a class of three, and a second class beside it
    t["three_way"] = _case(8, 6, [env([A_, B_, C_], ret=1.0), env([D_, B_], ret=0.0), env([B_, A_, C_], ret=3.0), env([A_, B_, C_], ret=2.0),
                                  env([D_, B_], ret=1.0), env([A_]), env([A_, D_, C_]), env([D_, A_, C_], ret=-1.0)])
    # ties in ret (0.0 and -0.0 tie under >): the lower env
    t["ret_ties"] = _case(4, 6, [env([D_]), env([A_, B_, C_], ret=-0.0), env([B_, A_, C_], ret=0.0), env([A_, B_, C_], ret=0.0)])
    # a NaN return ranks below every number, -inf included; two NaNs tie
    t["nan_ret"] = _case(4, 6, [env([A_, B_, C_], ret=np.nan), env([B_, A_, C_], ret=-np.inf), env([D_, A_], ret=np.nan),
                                env([D_, A_], ret=np.nan)])
    return t


def random_case(G, B, K, seed, key_last=1):
    """A seeded table of G groups of B beams: blocks from a small pool so that classes abound, orders shuffled, some dead envs,
    returns from a coarse grid with NaNs, n_blocks sometimes out of range, junk past the live slots."""
    rng = np.random.default_rng(seed)
    E = G * B
    xs = np.array([-1.5, -0.0, 0.0, 0.5, np.nextafter(0.5, 1.0)])
    pool = [(int(rng.integers(0, 2)), int(rng.integers(0, 4)), (float(rng.choice(xs)), 0.25 * int(rng.integers(1, 3)), 1.0, 0.0))
            for _ in range(5)]
    envs = []
    for e in range(E):
        if e % B and rng.random() < 0.6:                             # the blocks of an earlier env of the group, in another order
            src = envs[e - 1 - int(rng.integers(0, e % B))]
            blocks = [src["blocks"][i] for i in rng.permutation(len(src["blocks"]))]
            if blocks and rng.random() < 0.5:                        # ... keeping its last block
                i = blocks.index(src["blocks"][-1])
                blocks[i], blocks[-1] = blocks[-1], blocks[i]
            if blocks and rng.random() < 0.15:                       # ... or with one block swapped for another of the pool
                blocks[int(rng.integers(0, len(blocks)))] = pool[int(rng.integers(0, len(pool)))]
            tl = src["tl"] if rng.random() < 0.85 else src["tl"] ^ 1
        else:
            nb = int(rng.integers(0, K + 1)) if rng.random() < 0.8 else K
            blocks = [pool[int(rng.integers(0, len(pool)))] for _ in range(nb)]
            tl = int(rng.integers(0, 4))
        ret = float(rng.integers(-2, 3)) / 2.0 if rng.random() < 0.9 else np.nan
        envs.append(dict(blocks=blocks, tl=tl, live=int(rng.random() < 0.85), ret=ret))
    for env in envs:
        if len(env["blocks"]) == K and rng.random() < 0.3:
            env["nb"] = K + int(rng.integers(1, 4))                  # clamps to K
        elif not env["blocks"] and rng.random() < 0.3:
            env["nb"] = -int(rng.integers(1, 4))                     # clamps to 0
    return _case(B, K, envs, key_last=key_last)
