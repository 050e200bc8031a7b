"""GPU: bridges_td_target, bridges_td_target_rows and bridges_episode_stats reproduce, bit for bit, what they computed on
commit 02bfdb4 -- the last one on which each had a kernel of its own (tests/golden/make_twin_kernel_fixtures.py).  They now
launch k_td_target<PER_ROW> and k_episode_stats<1>, the kernels of bridges_td_target_select and of
bridges_episode_stats_by_class, so the tests that compare those entry points with each other compare one kernel with itself;
the recorded bits are the evidence that the fold changed nothing."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_twin_kernel_fixtures", os.path.join(GOLDEN, "make_twin_kernel_fixtures.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)

with open(G.FIXTURE) as _f:
    FIXTURE = json.load(_f)


@pytest.fixture(scope="module")
def td_now():
    return G.td_cases()


@pytest.fixture(scope="module")
def stats_now():
    return G.stats_cases()


def test_the_fixture_holds_the_cases_the_generator_runs(td_now, stats_now):
    assert FIXTURE["commit"] == "02bfdb4" and FIXTURE["gamma"] == G.GAMMA
    assert sorted(FIXTURE["td_target"]) == sorted(td_now) and len(td_now) == 16
    assert sorted(FIXTURE["episode_stats"]) == sorted(stats_now) and len(stats_now) == 6


@pytest.mark.parametrize("name", sorted(FIXTURE["td_target"]))
def test_td_target_gives_the_recorded_bits(name, td_now):
    want, got = FIXTURE["td_target"][name], td_now[name]
    assert got["argmax_row"] == want["argmax_row"]
    assert got["q_target"] == want["q_target"]
    assert got["sf_target"] == want["sf_target"]
    assert (want["sf_target"] is None) == name.startswith("sf_dim=0-")


@pytest.mark.parametrize("name", sorted(FIXTURE["episode_stats"]))
def test_episode_stats_gives_the_recorded_bits(name, stats_now):
    want, got = FIXTURE["episode_stats"][name], stats_now[name]
    assert got["out"] == want["out"] and want["out"][0] != 0            # (episodes were counted: the bits of 0.0 are 0)
    assert got["run"] == want["run"]
    assert got["counted"] == want["counted"]
