"""Plain reference of pc_env_rollout_sequences_value on the CPU oracle: sequences_reference.rollout's method, keeping every live step's
reward and the observation of every copy's last live step.

trace(): the rows replicated K times (copy m * K + k), OracleVecEnv.set_state once, raw_step H times, an ended copy frozen.  It is computed
once per key and never modified; discounted() forms ret_env / end_discount from it for a gamma with the header's recurrence -- one rounded
float64 multiplication and one rounded addition per step, which is what numpy's separate operations are --, combine() adds the bootstrap
and best() applies K22's rule.  The value is not recomputed here for the bit comparison: the GPU tests evaluate the policy step once on
the reference's end_obs; critic_f64() is the float64 MLP the tolerance check and the input counts use."""
import os

import numpy as np

import step_poses_reference as R      # (first: through conftest it puts the repository root on sys.path)
import sequences_reference as Q
import draw_reference as D

import oracle  # noqa: E402

from conftest import GOLDEN

RUNNING, TERMINATED, TRUNCATED = Q.RUNNING, Q.TERMINATED, Q.TRUNCATED
NONE, BOOT_RUNNING, BOOT_RUNNING_TRUNCATED = 0, 1, 2
MODES = {"none": NONE, "running": BOOT_RUNNING, "running_truncated": BOOT_RUNNING_TRUNCATED}
GAMMAS = (0.99, 0.5, 0.0, 1.0)
VALUE_KEYS = ("ret_env", "end_discount", "end_obs")
FRESH_SEED = 11           # the seeded fresh Agent of the config the trained fixture's D does not fit
FRESH_CRITIC_SCALE = 1.0  # ... and what its critic's output layer is multiplied by (1.0: as initialised)


def trace(name, n, state, actions, reward_scale=Q.REWARD_SCALE):
    """state / actions as sequences_reference.rollout takes them.  Returns a dict: rew float64 [H, M * K] (the float32 scaled reward of
    every step, widened), live bool [H, M * K] (the copy took that step), end_obs float32 [M, K, D], steps, gates, laps int32 and status
    uint8 [M, K], actions [M, H, K]."""
    M = len(state["px"])
    actions = np.asarray(actions)
    if actions.ndim == 2:
        actions = np.broadcast_to(actions, (M,) + actions.shape)
    H, K = actions.shape[1:]
    assert actions.min() >= 0 and actions.max() <= 8
    env = oracle.OracleVecEnv(R.track(name), M * K, n, threads=Q._THREADS)
    env.set_state(passed=0, destroyed=0, **{k: np.repeat(np.asarray(state[k]), K) for k in Q.STATE_KEYS})
    rew = np.zeros((H, M * K), np.float64)
    live = np.zeros((H, M * K), bool)
    steps, gates, laps = (np.zeros(M * K, np.int32) for _ in range(3))
    status = np.zeros(M * K, np.uint8)
    end_obs = None
    for t in range(H):
        a = actions[:, t, :].reshape(-1).astype(np.int64)
        obs, r, term, trunc = env.raw_step(a)
        if end_obs is None:
            end_obs = np.zeros((M * K, obs.shape[1]), np.float32)
        now = status == RUNNING
        live[t] = now
        rew[t] = (r * reward_scale).astype(np.float32).astype(np.float64)
        code = np.rint(r - 0.01 * np.isin(a, (0, 4, 5))).astype(np.int64)
        steps[now] += 1
        gates[now] += np.isin(code, R.GATE_CODES)[now]
        laps[now] += np.isin(code, Q.LAP_CODES)[now]
        status[now] = np.where(term, TERMINATED, np.where(trunc, TRUNCATED, RUNNING))[now]
        end_obs[now] = obs[now]
    return dict(rew=rew, live=live, end_obs=end_obs.reshape(M, K, -1), steps=steps.reshape(M, K), status=status.reshape(M, K),
                gates=gates.reshape(M, K), laps=laps.reshape(M, K), actions=actions)


def discount(rew, live, gamma):
    """The header's recurrence over rew, live [H, L]: (ret_env, end_discount) float64 [L]"""
    ret = np.zeros(rew.shape[1], np.float64)
    disc = np.ones(rew.shape[1], np.float64)
    g = np.float64(gamma)
    for t in range(rew.shape[0]):
        term = disc * rew[t]                       # one rounding
        ret = np.where(live[t], ret + term, ret)   # one rounding
        disc = np.where(live[t], disc * g, disc)
    return ret, disc


def discounted(tr, gamma):
    M, K = tr["status"].shape
    ret, disc = discount(tr["rew"], tr["live"], gamma)
    return ret.reshape(M, K), disc.reshape(M, K)


def bootstrapped(status, mode):
    """bool: the lanes whose status the mode covers"""
    if mode == NONE:
        return np.zeros(status.shape, bool)
    return (status == RUNNING) | ((status == TRUNCATED) if mode == BOOT_RUNNING_TRUNCATED else False)


def combine(ret_env, end_discount, value, status, mode):
    """ret float64: ret_env + end_discount * (double)value where the mode covers the status, else ret_env"""
    return np.where(bootstrapped(status, mode), ret_env + end_discount * np.asarray(value).astype(np.float64), ret_env)


def best(ret, actions):
    """K22's rule on ret [M, K] under actions [M, H, K]: (best_k int32, best_action int64, best_ret float64)"""
    M = ret.shape[0]
    k = ret.argmax(1).astype(np.int32)      # the first maximum
    return k, np.minimum(actions[np.arange(M), 0, k], 8).astype(np.int64), ret[np.arange(M), k]


_traces = {}


def pooled_trace(name, n, H, K):
    """(the 796 pooled rows, trace of the shared table(H, K)): computed once per key, never modified"""
    key = (name, n, H, K)
    if key not in _traces:
        s, _ = Q.pooled(name, n)
        _traces[key] = (s, trace(name, n, s, Q.table(H, K)))
    return _traces[key]


# ---- the critic --------------------------------------------------------------------------------------------------------------------------
def obs_dim(n):
    return 6 + len(range(0, 360, 360 // n))


def agent_for(n):
    """The test policy of a config, on the CPU: the trained fixture where its D fits, else an Agent of normal weights (fan-in scaled; biases 0.1 * normal) from
    default_rng(FRESH_SEED) whose critic output layer is multiplied by FRESH_CRITIC_SCALE.  Returns (agent, state dict as float64-ready numpy arrays)."""
    import torch
    import ppo_car_amd as pc
    Dn = obs_dim(n)
    f = np.load(os.path.join(GOLDEN, "policy_trained.npz"))
    if f["obs"].shape[1] == Dn:
        agent = pc.Agent(Dn, 9)
        agent.load_state_dict({k: torch.from_numpy(f[k.replace(".", "_")]) for k in agent.state_dict()})
    else:      # numpy's generator, not torch's initialiser: the same weights on every machine
        rng = np.random.default_rng(FRESH_SEED)
        agent = pc.Agent(Dn, 9)
        sd = {}
        for k, v in agent.state_dict().items():
            scale = 0.1 if k.endswith("bias") else 1.0 / np.sqrt(v.shape[1])
            sd[k] = torch.from_numpy((rng.standard_normal(tuple(v.shape)) * scale).astype(np.float32))
        sd["critic.2.weight"] *= FRESH_CRITIC_SCALE
        sd["critic.2.bias"] *= FRESH_CRITIC_SCALE
        agent.load_state_dict(sd)
    return agent, {k: v.detach().numpy().copy() for k, v in agent.state_dict().items()}


def critic_f64(weights, obs):
    """(logits, value) of the float64 MLP over obs [..., D]"""
    flat = np.asarray(obs).reshape(-1, np.asarray(obs).shape[-1])
    L, V = D.mlp_f64(weights, flat)
    return L, V.reshape(np.asarray(obs).shape[:-1])


# ---- how much the critic changes the choice ----------------------------------------------------------------------------------------------
# Rows of the 796 whose best_k differs between bootstrap none and running at gamma 0.99, K = 64, with the float64 critic: per config at
# H = 4 and H = 12.  The floor: 20 rows at one of the two horizons on every config.
RICH_GAMMA, RICH_FLOOR = 0.99, 20
RICH_COUNTS = {("big_track", 16): {4: 225, 12: 189}, ("track", 12): {4: 295, 12: 218}, ("oval64", 16): {4: 309, 12: 249}}


def richness(name, n, H, K=Q.K_REF):
    _, tr = pooled_trace(name, n, H, K)
    _, w = agent_for(n)
    _, v = critic_f64(w, tr["end_obs"])
    ret_env, disc = discounted(tr, RICH_GAMMA)
    plain = best(ret_env, tr["actions"])[0]
    boot = best(combine(ret_env, disc, v, tr["status"], BOOT_RUNNING), tr["actions"])[0]
    return int((plain != boot).sum())
