"""The off-menu ray counts on the CPU: the oracle pinned, bit for bit, to fixtures recorded from the unmodified reference at the seven
counts of tests/ray_counts_reference.py (tests/golden/make_golden.py rays), what those fixtures must contain for the GPU tests to
mean something, and the harvested oracle states those tests step."""
import os

import numpy as np
import pytest

import oracle
import ray_counts_reference as rc
from conftest import GOLDEN, TRACKS
from ray_counts_reference import CASE_IDS, CASES, STATE

cases = pytest.mark.parametrize("track,n", CASES, ids=CASE_IDS)


def test_the_table_is_what_the_reference_builds():
    for n, step, R, D, col, track in rc.TABLE:
        assert oracle.ray_count(n) == R == len(range(0, 360, 360 // n))
        assert rc.geometry(n) == (step, R, list(col))
    assert [n for _, n in CASES] == [4, 5, 7, 11, 31, 90, 181]
    assert len(rc.geometry(7)[2]) == 7 and len(rc.geometry(11)[2]) == 6 and rc.geometry(7)[1] == 8      # nc = 7, nc = 6, R > n
    assert min(c for c in rc.geometry(90)[2] if c) < 64 <= max(rc.geometry(90)[2])                      # rays on both sides of the mask
    assert [c for c in rc.geometry(181)[2] if c >= 64] == [90, 135, 180]
    # the look-alikes: the rays of 12 / 32 nominal rays in number (and, for 31, in angle), other collision rays
    assert rc.geometry(11)[1] == rc.geometry(12)[1] and rc.geometry(11)[0] != rc.geometry(12)[0]
    assert rc.geometry(31)[:2] == rc.geometry(32)[:2] and rc.geometry(31)[2] != rc.geometry(32)[2]


@cases
def test_fixture_size_and_geometry(track, n):
    assert os.path.getsize(rc.fixture_path(track, n)) <= os.path.getsize(f"{GOLDEN}/env_track_n12.npz")
    g = rc.load(track, n)
    tr = oracle.Track(TRACKS[track])
    assert int(g["num_rays_nominal"]) == n and g["step_obs"].shape[2] == 6 + rc.geometry(n)[1]
    assert np.array_equal(tr.walls, g["walls"]) and np.array_equal(tr.gates, g["gates"])
    assert np.array_equal(np.array([tr.start_x, tr.start_y, 0.0, 0.0, tr.start_rot]), g["reset_state"])
    assert g["action"].shape[1] == 6                                      # six policies
    env = oracle.OracleVecEnv(tr, 2, num_rays=n)
    obs = env.reset()
    assert obs.dtype == np.float32 and np.array_equal(obs[0], g["reset_obs"]) and np.array_equal(obs[1], g["reset_obs"])


@cases
def test_teacher_forced_step(track, n):
    """Every recorded transition: inject the reference pre-state, apply the action, compare all."""
    g = rc.flat(rc.load(track, n))
    M = len(g["action"])
    env = oracle.OracleVecEnv(oracle.Track(TRACKS[track]), M, num_rays=n)
    env.set_state(destroyed=0, **{k: g[f"pre_{k}"] for k in STATE})
    obs, rew, term, trunc = env.raw_step(g["action"])
    assert np.array_equal(obs, g["step_obs"])
    assert np.array_equal(rew, g["reward"])
    assert np.array_equal(term, g["terminated"])
    assert np.array_equal(trunc, g["truncated"])
    for k in STATE:
        assert np.array_equal(getattr(env, k), g[f"post_{k}"]), k


@cases
def test_free_running_vector_env(track, n):
    """Replay the recorded action streams from reset through the vector-env call (auto-reset + reward scaling)."""
    g = rc.load(track, n)
    act = g["action"]
    T, N = act.shape
    env = oracle.OracleVecEnv(oracle.Track(TRACKS[track]), N, num_rays=n, reward_scaling=float(g["reward_scaling"]))
    env.reset()
    n_done = 0
    for t in range(T):
        for k in STATE:
            assert np.array_equal(getattr(env, k), g[f"pre_{k}"][t]), (t, k)
        obs, rew, term, trunc, fin = env.step(act[t], want_final_obs=True)
        assert np.array_equal(obs, g["ret_obs"][t]), t
        assert np.array_equal(fin, g["step_obs"][t]), t
        assert np.array_equal(rew, g["reward_scaled"][t]), t
        assert np.array_equal(term, g["terminated"][t]), t
        assert np.array_equal(trunc, g["truncated"][t]), t
        n_done += int(term.sum() + trunc.sum())
    assert n_done > 0


@cases
def test_fixture_coverage(track, n):
    g = rc.flat(rc.load(track, n))
    assert g["terminated"].sum() >= 5
    assert (g["post_passed"] > g["pre_passed"]).sum() >= 10
    assert ((g["reward"] > 0.5) & ~g["terminated"]).sum() >= 10                       # ... and they paid
    assert {0, 1, 6, 7} <= set(np.unique(g["action"]).tolist())                        # forward and the three reversing actions
    assert ((g["wall_margin"] > rc.MARGIN_PX) & (g["gate_margin"] > rc.MARGIN_PX)).mean() >= 0.99
    # the margins are those of the collision rays of THIS count (recomputed by the oracle's single-ray form on a few rows)
    tr = oracle.Track(TRACKS[track])
    idx = np.arange(0, len(g["action"]), max(1, len(g["action"]) // 40))
    wd = rc.collision_ray_distances(tr.walls, g["post_px"][idx], g["post_py"][idx], g["post_rot"][idx], n)
    assert np.array_equal(np.abs(wd - 10.0).min(1), g["wall_margin"][idx])


def test_n181_crashes_through_the_rays_past_the_mask_alone():
    """A car that reverses into a wall is seen by ray 180 (or 135) alone: collision rays whose index the 64-bit mask cannot hold."""
    g = rc.flat(rc.load("track", 181))
    hi = rc.high_ray_only_crashes(g, "track", 181)
    assert hi.sum() >= 5, int(hi.sum())
    assert set(np.unique(g["action"][hi]).tolist()) <= {1, 6, 7}


def test_n7_ray_7_reads_a_wall_and_the_step_goes_on():
    """Ray 7 (357 degrees) is measured and observed, but no collision ray: below 10 px it must not end the episode."""
    g = rc.flat(rc.load("big_track", 7))
    assert ((g["step_obs"][:, 6 + 7] * 1000.0 < 10.0) & ~g["terminated"]).sum() >= 1


@cases
def test_harvest(track, n):
    g = rc.harvest(track, n)
    M = len(g["action"])
    assert 1500 <= M <= 2048 and g["step_obs"].shape == (M, 6 + rc.geometry(n)[1])
    assert g["terminated"].sum() >= 100 and (g["post_passed"] > g["pre_passed"]).sum() >= 100
    assert g["truncated"].sum() >= 32 and (g["pre_time_step"] == 999).sum() == 64
    assert (~(g["terminated"] | g["truncated"]) & (g["reward"] < 0.5)).sum() >= 1       # plain rows too
    assert ((g["wall_margin"] > rc.MARGIN_PX) & (g["gate_margin"] > rc.MARGIN_PX)).mean() > 0.99
    assert set(np.unique(g["action"]).tolist()) == set(range(9))
    if n == 31:     # a kernel that takes 31 nominal rays for 32 fails on these rows
        assert g["differs_at_32"].sum() >= 50, int(g["differs_at_32"].sum())
    if n == 181:
        k = g["n_high_ray_only"]
        assert k >= 5 and g["terminated"][:k].all()
    if n in (90, 181):      # (at n = 90 the rear ray is ray 44: only a crash sideways, through ray 66 alone, is past the mask)
        hi = rc.high_ray_only_crashes(g, track, n)
        print(f"n = {n}: {int(hi.sum())} crashes through rays 64 and up alone, {int((g['terminated'] & ~hi).sum())} others")
        assert hi.sum() >= (1 if n == 90 else 10) and (g["terminated"] & ~hi).sum() >= 50


# ---- what the stateless kernels' recipes must reach, at the counts their GPU tests add (the reference modules' own thresholds) --------
@pytest.mark.parametrize("n", [5, 7, 11, 90, 181])
def test_step_poses_recipes_at_the_new_counts(n):
    import step_poses_reference as R
    track = rc.TRACK_OF[n]
    rows, acts = R.all_actions(R.edge_states(track))
    ref = R.step(track, n, rows, acts)
    c = R.counts(ref, ref["next_gate"])
    assert c["terminated"] > 0 and c["truncated"] > 0
    rows, acts = R.all_actions(R.near_gate_states(track))
    ref = R.step(track, n, rows, acts)
    c = R.counts(ref, ref["next_gate"])
    assert c["gates"] > 0 and c["laps"] > 0 and c["truncated"] > 0 and c["terminated"] == 0


@pytest.mark.parametrize("n", [7, 181])
def test_safe_action_shares_at_the_new_counts(n):
    """safe_actions_reference.SHARES of the pre-crash rows -- empty, partial and full masks -- at the depths the GPU tests run"""
    import safe_actions_reference as S
    s, ref = S.reference(rc.TRACK_OF[n], n, "pre_crash", 2)
    M = len(s["px"])
    assert M >= 200
    for m in ref[:2]:
        assert all(c >= need * M for c, need in zip(S.classes(m), S.SHARES)), S.classes(m)


@pytest.mark.parametrize("n", [11, 90])
def test_sequence_inputs_at_the_new_counts(n):
    """sequences_reference.NEED, every share of it, at the shape it is stated for: (K, H) = (64, 12), the same rows at the new counts.
    The GPU tests at these counts score (K, H) = (70, 3), the shape their issue sets.  There NEED's shares of the (state, sequence) pairs
    and its mixed-status and drawn-best rows hold too, and are asserted; its 40 rows with a unique best sequence are NOT reached in three
    steps (24 rows at 11 nominal rays, 33 at 90: short sequences tie), so best_k / best_action are held to the oracle on fewer
    tie-free rows there than at twelve steps.  That count is printed, not asserted."""
    import sequences_reference as Q
    track = rc.TRACK_OF[n]
    Q.meets(*Q.counts(track, n))
    c, pairs, lap_pairs = Q.counts(track, n, 3, 70)
    print(f"n = {n} at (K, H) = (70, 3): {c}")
    for k in Q.COUNT_KEYS:
        if k != "unique_max_rows":
            need = Q.NEED[k] * (lap_pairs if k == "lap" else pairs) if isinstance(Q.NEED[k], float) else Q.NEED[k]
            assert c[k] >= need, (k, c[k], need)
