"""Episode statistics: gymnasium's RecordEpisodeStatistics (episodic return and length) plus gates and laps per episode, computed
on the device by the K3e kernels (include/ppocar.h pc_episode_stats / pc_gae_episodes).

Per env the state is a carry (return so far, length so far, gates, laps) in float64, [4, N]; length -1 = the start of the episode in
progress was not observed (forget(), a checkpoint without statistics): that episode is dropped when it closes.  Each update()
ACCUMULATES into an `out` [7, N] float64 (finished episodes, sum of scaled returns, of lengths, gates, laps; min / max scaled
return) that new_out() / clear() initialise.  Returns are stored scaled (the env's r * reward_scaling) and reported unscaled, by the
convention of charts/avg_reward."""
import torch

from ._capi import PC_EPISODE_BUFFER, PC_EPISODE_STEPS, check, lib

LAYOUTS = {"buffer": PC_EPISODE_BUFFER, "steps": PC_EPISODE_STEPS}
EPISODE_MEAN_KEYS = ("charts/episodic_return", "charts/episodic_return_min", "charts/episodic_return_max", "charts/episodic_length",
                     "charts/gates_per_episode", "charts/laps_per_episode")


class EpisodeStats:
    def __init__(self, n_envs, reward_scaling, device):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("EpisodeStats runs the HIP episode kernels: the device must be a GPU")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.num_envs = int(n_envs)
        self.reward_scaling = float(reward_scaling)
        self.carry = torch.zeros(4, self.num_envs, dtype=torch.float64, device=self.device)   # a reset env: an observed start
        self._init = torch.tensor([0.0, 0.0, 0.0, 0.0, 0.0, float("inf"), float("-inf")], dtype=torch.float64,
                                  device=self.device).reshape(7, 1).expand(7, self.num_envs).contiguous()
        self.out = self.new_out()

    def new_out(self):
        return self._init.clone()

    def clear(self, out=None):
        """Reinitialise `out` (default: self.out) in place: no episode finished."""
        (self.out if out is None else out).copy_(self._init)

    def reset(self):
        """Every env was reset: the episodes in progress start here."""
        self.carry.zero_()

    def forget(self):
        """The episodes in progress have an unknown history (the env state was injected): drop them when they close."""
        self.carry.zero_()
        self.carry[1].fill_(-1.0)

    def _check(self, t, T, what):
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == T * self.num_envs):
            raise ValueError(f"{what}: need a contiguous float32 CUDA tensor with {T * self.num_envs} elements, got "
                             f"{tuple(t.shape)} {t.dtype} {t.device}")
        return t.data_ptr()

    def update(self, rew, term, trunc, last_term=None, last_trunc=None, layout="buffer", out=None):
        """rew, term, trunc [T, N] (or [N]: T = 1).  layout "buffer": step t's flags in row t + 1 and step T - 1's in last_term /
        last_trunc [N]; "steps": flags[t] belong to rew[t] (what VecCarEnv.step / step_many return)."""
        T = rew.numel() // self.num_envs
        lay = LAYOUTS[layout]
        out = self.out if out is None else out
        lt = self._check(last_term, 1, "last_term") if lay == PC_EPISODE_BUFFER else None
        ltr = self._check(last_trunc, 1, "last_trunc") if lay == PC_EPISODE_BUFFER else None
        check(lib.pc_episode_stats(self.device.index, self._check(rew, T, "rew"), self._check(term, T, "term"),
                                   self._check(trunc, T, "trunc"), lt, ltr, T, self.num_envs, lay, self.reward_scaling,
                                   self.carry.data_ptr(), out.data_ptr(), torch.cuda.current_stream(self.device).cuda_stream),
              "pc_episode_stats")
        return out

    def totals(self, out=None):
        """Reduce `out` over envs in a fixed order (no host synchronisation) -> float64 [7]: episodes, the sums of scaled return,
        length, gates and laps, min and max scaled return."""
        out = self.out if out is None else out
        return torch.cat([out[:5].sum(dim=1), out[5].min().reshape(1), out[6].max().reshape(1)])

    def summary_from_totals(self, tot):
        """float64 [7] totals (possibly all-reduced over ranks) -> dict of 0-d device tensors: means per finished episode (NaN where
        none finished), returns unscaled."""
        n = tot[0]
        s = self.reward_scaling
        return {"episodes": n, "return": tot[1] / n / s, "return_min": tot[5] / s, "return_max": tot[6] / s,
                "length": tot[2] / n, "gates": tot[3] / n, "laps": tot[4] / n}

    def summary(self, out=None):
        return self.summary_from_totals(self.totals(out))

    def state_dict(self):
        return {"carry": self.carry.clone(), "reward_scaling": self.reward_scaling}

    def load_state_dict(self, sd):
        self.carry.copy_(sd["carry"])


def episode_scalars(tot, reward_scaling):
    """Host totals [7] (EpisodeStats.totals(), tolist()) -> run_epoch's keys.  The means are None in an epoch without a finished episode."""
    n, s = tot[0], float(reward_scaling)
    if n == 0:
        return {"charts/episodes": 0, **{k: None for k in EPISODE_MEAN_KEYS}}
    return {"charts/episodes": int(n), "charts/episodic_return": tot[1] / n / s, "charts/episodic_return_min": tot[5] / s,
            "charts/episodic_return_max": tot[6] / s, "charts/episodic_length": tot[2] / n, "charts/gates_per_episode": tot[3] / n,
            "charts/laps_per_episode": tot[4] / n}


def to_host(summary):
    """0-d tensors -> Python floats (synchronises); the means of an epoch without a finished episode are None."""
    d = {k: float(v) for k, v in summary.items()}
    if d["episodes"] == 0:
        for k in ("return", "return_min", "return_max", "length", "gates", "laps"):
            d[k] = None
    return d
