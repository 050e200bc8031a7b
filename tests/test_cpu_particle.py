"""CPU-only: the reference of bridges_particle_select (tests/particle_ref.py) -- against its brute-force second statement, the
twins its probes must reject, the census of the probes, the two exact properties of the rule, the systematic count property and
the share of undecided draws -- and the host side: the argument checks of ops.particle_select, which need no device."""
import math

import numpy as np
import pytest
import torch

import particle_ref as P

NAN, INF = float("nan"), float("inf")
ALL = P.all_probes()


# --------------------------------------------------------------------------------------------------------------------- the rule
@pytest.mark.parametrize("name", sorted(ALL))
def test_reference_equals_brute_force(name):
    assert P.agrees_with_brute_force(ALL[name]), name


@pytest.mark.parametrize("twin", P.TWINS)
def test_every_defective_twin_is_rejected_by_the_named_probes(twin):
    named = {**P.named_probes(), **P.nonfinite_probes()}
    rejected = [k for k, c in named.items() if P.differs(P.reference(c), P.reference(c, twin=twin), c)]
    assert rejected, twin


def test_the_rule_itself_passes_its_own_comparison():
    for c in ALL.values():
        assert not P.differs(P.reference(c), P.reference(c), c)


def test_census_of_the_named_probes_is_the_full_case_list():
    seen = set()
    for c in {**P.named_probes(), **P.nonfinite_probes()}.values():
        seen |= P.census(c)
    assert seen == set(P.CENSUS), (set(P.CENSUS) - seen, seen - set(P.CENSUS))


def test_exact_probes_have_integer_prefix_sums_and_sit_on_boundaries():
    on_boundary = 0
    for name, c in P.exact_probes().items():
        ref = P.reference(c)
        live = ref["live"] == 1
        assert (ref["W"][c["live"] == 1] == 1.0).all(), name
        assert np.array_equal(ref["p_sel"][live & (ref["margin_row"] < INF)], np.full((live & (ref["margin_row"] < INF)).sum(), 0.125))
        on_boundary += int((ref["margin_parent"] == 0).sum()) + int((ref["margin_row"] == 0).sum())
    assert on_boundary > 100


def test_without_resampling_no_particle_moves():
    """T_r = +inf, elite off, every env a parent: src is the identity, whatever u_res."""
    for B in (1, 2, 3, 5, 7, 16):
        for seed in range(3):
            c = P.random_probe(6, B, 1.0, INF, False, seed=50 + seed, all_parents=True)
            c["u_res"][:3] = [0.0, 1.0 - 2.0 ** -24, 2.0 ** -149]
            ref = P.reference(c)
            assert ref["live"].all() and np.array_equal(ref["src"], np.arange(6 * B)), (B, seed)
            assert np.array_equal(ref["ess"], np.full(6, float(B)))


def test_width_1_with_the_elite_is_the_beam_select():
    import beam_ref as BR
    for seed in range(4):
        c = P.random_probe(40, 1, 0.5, 1.0, True, seed=70 + seed)              # finite ret, disc > 0
        ref, want = P.reference(c), BR.reference(c)
        for k in BR.OUTPUTS:
            assert ref[k].astype(want[k].dtype).tobytes() == want[k].tobytes(), k
        assert 0 < ref["live"].sum() < 40                                    # dead and rowless envs are among them
        assert np.array_equal(ref["p_sel"], ref["live"].astype(np.float64))


def test_systematic_count_property():
    """With every draw of a group decided and the elite off, each parent receives floor or ceil of B W_p / total slots."""
    groups = 0
    for name, c in P.random_probes().items():
        if c["elite"]:
            continue
        ref = P.reference(c)
        B = c["B"]
        for g in range(len(c["u_res"])):
            sl = slice(g * B, (g + 1) * B)
            if not ref["live"][sl].all() or not ref["decided"][sl].all():
                continue
            W = ref["W"][sl]
            share = B * W / W.sum()
            counts = np.bincount(ref["src"][sl] - g * B, minlength=B)
            assert ((counts >= np.floor(share)) & (counts <= np.ceil(share))).all(), (name, g, counts, share)
            groups += 1
    assert groups > 40


def test_undecided_share_of_the_random_probes():
    """A condition on the inputs (the seeds are fixed): at most 1 slot in 1000 lies within MARGIN of a boundary."""
    slots = undecided = 0
    for c in P.random_probes().values():
        ref = P.reference(c)
        slots += len(ref["decided"])
        undecided += int((~ref["decided"]).sum())
    assert slots > 1000 and undecided * 1000 <= slots, (undecided, slots)


def test_bounds_are_those_of_the_derivation():
    assert P.p_sel_bound(1.0, 300) == (2.0 ** -23 + 610 * 2.0 ** -53) + 2.0 ** -149
    assert P.ess_bound(16.0, 16) == 2 * 118 * 2.0 ** -53 * 16.0
    assert math.isclose(P.MARGIN, 2.0 ** -40)


# ----------------------------------------------------------------------------------------------------------------- ops arguments
def _args(B=2, G=3, n=10):
    E = G * B
    return dict(seg=(torch.zeros(E, dtype=torch.int32), torch.full((E,), n, dtype=torch.int32)), q=torch.zeros(n), width=B,
                live=torch.ones(E, dtype=torch.uint8), ret=torch.zeros(E, dtype=torch.float64), disc=torch.ones(E, dtype=torch.float64),
                idx=torch.arange(n), cand_offset=torch.zeros(E, dtype=torch.int32), u_act=torch.zeros(E), u_res=torch.zeros(G),
                temperature=1.0, resample_temperature=1.0)


def test_particle_select_args_accepts_and_refuses_in_words():
    from bridges_hip import ops
    lo, hi, E, B, G, n = ops.particle_select_args(**_args())
    assert (E, B, G, n) == (6, 2, 3, 10)
    ops.particle_select_args(**dict(_args(), resample_temperature=INF, rep=torch.zeros(6, dtype=torch.int32)))
    ops.particle_select_args(**dict(_args(), seg=torch.zeros(7, dtype=torch.int32)))                 # a prefix-sum array
    bad = [dict(width=0), dict(width=17), dict(width=4), dict(temperature=0.0), dict(temperature=INF), dict(temperature=NAN),
           dict(temperature=-1.0), dict(resample_temperature=0.0), dict(resample_temperature=NAN), dict(resample_temperature=-INF),
           dict(q=torch.zeros(10, dtype=torch.float64)), dict(idx=torch.arange(10, dtype=torch.int32)), dict(idx=torch.arange(9)),
           dict(live=torch.ones(6, dtype=torch.bool)), dict(ret=torch.zeros(6)), dict(disc=torch.ones(5, dtype=torch.float64)),
           dict(u_act=torch.zeros(5)), dict(u_act=torch.zeros(6, dtype=torch.float64)), dict(u_res=torch.zeros(6)),
           dict(u_res=torch.zeros(6)[::2]), dict(rep=torch.zeros(6, dtype=torch.int64)), dict(cand_offset=torch.zeros(5, dtype=torch.int32)),
           dict(out=dict(src=torch.zeros(6, dtype=torch.int32)))]
    for kw in bad:
        with pytest.raises(ValueError, match="particle_select"):
            ops.particle_select_args(**dict(_args(), **kw))


def test_entry_point_is_declared_with_its_rule():
    import os
    from bridges_hip import abi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "bridges_hip.h")).read()
    assert "int bridges_particle_select(int32_t E, int32_t B, int32_t n_rows," in header
    assert "first parent\n *     p with C_p > t_k (strict)" in header and "no particle moves" in header
    assert "bridges_particle_select" in abi.EXPORTED_SYMBOLS and len(abi.SIGNATURES["bridges_particle_select"]) == 26


# ------------------------------------------------------------------------------------------------------------------ command line
def test_a_plain_parse_is_unchanged_and_the_flags_need_their_option():
    from robotoddler.training import successor_dqn as S
    parse = lambda *argv: vars(S.build_parser().parse_args(list(argv)))
    plain = parse()
    new = {"eval_particles", "eval_particle_temperature", "eval_particle_resample_temperature", "eval_particle_no_elite",
           "eval_particle_merge", "search_particles", "search_temperature", "search_resample_temperature"}
    assert not new & set(plain)                                              # SUPPRESS: a plain parse is as it was
    S.check_eval_particles(plain)
    assert S.eval_particles_from_args(plain) is None and S.search_from_args(plain) == {}
    ok = parse("--num_envs", "64", "--search_every", "10")
    assert S.search_from_args(ok) == dict(search_every=10, search_width=8, search_merge=False)     # today's flags: today's result
    for flag, value in (("--eval_particle_temperature", "0.5"), ("--eval_particle_resample_temperature", "inf"),
                        ("--eval_particle_no_elite", None), ("--eval_particle_merge", None)):
        with pytest.raises(SystemExit, match="--eval_particles B"):
            S.check_eval_particles(parse("--num_envs", "64", flag, *([value] if value else [])))
    for flag, value in (("--search_particles", None), ("--search_temperature", "0.5"), ("--search_resample_temperature", "2")):
        with pytest.raises(SystemExit, match="--search_every N"):
            S.check_search(parse("--num_envs", "64", flag, *([value] if value else [])))


def test_command_line_of_the_evaluation():
    from robotoddler.training import successor_dqn as S
    parse = lambda *argv: vars(S.build_parser().parse_args(list(argv)))
    base = ("--num_envs", "64", "--eval_envs", "8", "--eval_particles", "8")
    got = S.eval_particles_from_args(parse(*base, "--eval_particle_temperature", "0.5"))
    assert got == dict(width=8, temperature=0.5, resample_temperature=None, elite=True, merge=False)
    got = S.eval_particles_from_args(parse(*base, "--eval_particle_temperature", "0.5", "--eval_particle_resample_temperature", "inf",
                                           "--eval_particle_no_elite", "--eval_particle_merge"))
    assert got == dict(width=8, temperature=0.5, resample_temperature=INF, elite=False, merge=True)
    with pytest.raises(SystemExit, match="--eval_particle_temperature T"):
        S.check_eval_particles(parse(*base))
    with pytest.raises(SystemExit, match="--eval_beam"):
        S.check_eval_particles(parse(*base, "--eval_particle_temperature", "0.5", "--eval_beam", "4"))
    for bad in ("0", "-1", "inf", "nan"):
        with pytest.raises(SystemExit, match="finite and > 0"):
            S.check_eval_particles(parse(*base, "--eval_particle_temperature", bad))
    for bad in ("0", "-2", "nan"):
        with pytest.raises(SystemExit, match="resample_temperature"):
            S.check_eval_particles(parse(*base, "--eval_particle_temperature", "1", "--eval_particle_resample_temperature", bad))
    # wherever check_eval_beam refuses: the width, the single-env loop, no evaluation env
    with pytest.raises(SystemExit, match="--eval_particles must be 1..16"):
        S.check_eval_particles(parse("--num_envs", "64", "--eval_envs", "8", "--eval_particles", "17", "--eval_particle_temperature", "1"))
    with pytest.raises(SystemExit, match="--num_envs"):
        S.check_eval_particles(parse("--eval_envs", "8", "--eval_particles", "4", "--eval_particle_temperature", "1"))
    with pytest.raises(SystemExit, match="--eval_envs"):
        S.check_eval_particles(parse("--num_envs", "64", "--eval_envs", "0", "--eval_particles", "4", "--eval_particle_temperature", "1"))
    with pytest.raises(SystemExit, match="--eval_particle_temperature T"):
        S.main(["--num_envs", "64", "--eval_particles", "4"])                 # refused before the GPU is asked for
    assert "particle_success_rate" in S.build_parser().format_help()


def test_command_line_of_the_search_in_training():
    from robotoddler.training import successor_dqn as S
    parse = lambda *argv: vars(S.build_parser().parse_args(list(argv)))
    base = ("--num_envs", "64", "--search_every", "10", "--search_particles")
    assert S.search_from_args(parse(*base, "--search_temperature", "0.5")) == dict(
        search_every=10, search_width=8, search_merge=False, search_sampler="particles", search_temperature=0.5)
    assert S.search_from_args(parse(*base, "--search_temperature", "0.5", "--search_resample_temperature", "inf", "--search_width", "4")) == dict(
        search_every=10, search_width=4, search_merge=False, search_sampler="particles", search_temperature=0.5,
        search_resample_temperature=INF)
    with pytest.raises(SystemExit, match="--search_temperature T"):
        S.check_search(parse(*base))
    for flag in ("--search_temperature", "--search_resample_temperature"):
        with pytest.raises(SystemExit, match="--search_particles"):
            S.check_search(parse("--num_envs", "64", "--search_every", "10", flag, "0.5"))
    for bad in ("0", "-1", "inf", "nan"):
        with pytest.raises(SystemExit, match="finite and > 0"):
            S.check_search(parse(*base, "--search_temperature", bad))
    for bad in ("0", "nan"):
        with pytest.raises(SystemExit, match="resample_temperature"):
            S.check_search(parse(*base, "--search_temperature", "1", "--search_resample_temperature", bad))


# ----------------------------------------------------------------------------------------------------------------------- VecDQN
def test_construction_and_checkpoint_of_the_sampler(monkeypatch, tmp_path):
    from test_cpu_beam_trace import _host_agent, _stand_in_env
    mk = lambda **kw: _host_agent(monkeypatch, _stand_in_env(), per_env_tasks=True, **kw)
    plain, beam = mk(), mk(search_every=5)
    assert plain.search_sampler is None and beam.search_sampler is None and beam.search_gen is None
    a = mk(search_every=5, search_sampler="particles", search_temperature=0.5)
    assert (a.search_sampler, a.search_temperature, a.search_resample_temperature) == ("particles", 0.5, 0.5)
    b = mk(search_every=5, search_sampler="particles", search_temperature=0.5, search_resample_temperature=INF)
    assert b.search_resample_temperature == INF
    for kw, word in ((dict(search_sampler="particles", search_temperature=1.0), "need search_every"),
                     (dict(search_temperature=1.0), "need search_every"), (dict(search_resample_temperature=1.0), "need search_every"),
                     (dict(search_every=2, search_temperature=1.0), "search_sampler='particles'"),
                     (dict(search_every=2, search_resample_temperature=1.0), "search_sampler='particles'"),
                     (dict(search_every=2, search_sampler="gumbel", search_temperature=1.0), "'particles' or None"),
                     (dict(search_every=2, search_sampler="particles"), "search_temperature"),
                     (dict(search_every=2, search_sampler="particles", search_temperature=0.0), "finite and > 0"),
                     (dict(search_every=2, search_sampler="particles", search_temperature=INF), "finite and > 0"),
                     (dict(search_every=2, search_sampler="particles", search_temperature=NAN), "finite and > 0"),
                     (dict(search_every=2, search_sampler="particles", search_temperature=1.0, search_resample_temperature=0.0), "> 0"),
                     (dict(search_every=2, search_sampler="particles", search_temperature=1.0, search_resample_temperature=NAN), "> 0")):
        with pytest.raises(ValueError) as e:
            mk(**kw)
        assert word in str(e.value), (kw, str(e.value))
    # the keys ride in save_extra only with the option; another setting is refused in words; the other streams do not move
    p0, p1, p2 = (str(tmp_path / n) for n in ("plain.pt", "beam.pt", "particles.pt"))
    plain.save_extra(p0, lockstep=1)
    beam.save_extra(p1, lockstep=2)
    for path in (p0, p1):
        assert not {"search_sampler", "search_gen"} & set(torch.load(path, weights_only=True))
    assert beam.search_gen is None                                          # saving a plain run makes no stream
    before = (a.sample_gen.get_state().clone(), a.explore_gen.get_state().clone())
    gen = a._search_generator()
    assert gen is a._search_generator() and gen.initial_seed() != a.sample_gen.initial_seed()
    drawn = torch.rand(5, generator=gen)
    assert torch.equal(a.sample_gen.get_state(), before[0]) and torch.equal(a.explore_gen.get_state(), before[1])
    a.save_extra(p2, lockstep=8)
    blob = torch.load(p2, weights_only=True)
    assert tuple(blob["search_sampler"]) == ("particles", 0.5, 0.5) and "search_gen" in blob
    again = mk(search_every=5, search_sampler="particles", search_temperature=0.5)
    first = torch.rand(5, generator=again._search_generator())
    assert torch.equal(first, drawn)                                        # the same seed: the same stream
    assert again.load_extra(p2) == dict(lockstep=8)
    nxt = torch.rand(5, generator=again._search_generator())
    assert torch.equal(nxt, torch.rand(5, generator=gen)) and not torch.equal(nxt, drawn)        # continues where the file stood
    for other in (beam, plain, b, mk(search_every=5, search_sampler="particles", search_temperature=0.25)):
        with pytest.raises(ValueError, match="search_sampler"):
            other.load_extra(p2)
    with pytest.raises(ValueError, match="search_sampler"):
        a.load_extra(p1)
    assert beam.load_extra(p1) == dict(lockstep=2) and plain.load_extra(p0) == dict(lockstep=1)


def test_particle_search_refuses_its_temperatures_before_anything_runs(monkeypatch):
    from test_cpu_beam_trace import _host_agent, _stand_in_env
    a = _host_agent(monkeypatch, _stand_in_env(), per_env_tasks=True)
    for kw in (dict(temperature=0.0), dict(temperature=INF), dict(temperature=NAN), dict(temperature=1.0, resample_temperature=0.0),
               dict(temperature=1.0, resample_temperature=NAN)):
        with pytest.raises(ValueError, match="particle_search"):
            a.particle_search(_stand_in_env(), 4, **kw)
    with pytest.raises(ValueError, match=r"particle_search\(\) needs an env of its own"):
        a.particle_search(a.env, 4, 1.0)
    with pytest.raises(ValueError, match=r"particle_search\(width=17\)"):
        a.particle_search(_stand_in_env(), 17, 1.0)
