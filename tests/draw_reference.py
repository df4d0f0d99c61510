"""A plain reference of the library's categorical draw (include/ppocar.h, "The stream"): numpy only, no kernel code.

  philox4x32_10   the Philox-4x32-10 block function of Salmon et al. (Random123), vectorised
  philox_words    the block a draw reads: counter = (idx lo, idx hi, block lo, block hi), key = (seed lo, seed hi), block = offset >> 2
  uniform         draw number `offset` of element `idx`: word offset & 3 of that block, mapped to float32 by the library's own
                  expression in numpy float32, operation for operation -- the value is EXACT, not close
  mlp_f64         Agent's two one-hidden-layer MLPs (model.py:12-32) in float64
  draw_f64        float64 softmax, inclusive CDF, inverse-CDF action, log-probs, entropy and each element's distance to the nearest
                  bin boundary (the elements a float32 CDF may legitimately decide the other way)
"""
import numpy as np

_M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)
_MUL0, _MUL1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_KEY0, _KEY1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)

U_MAX = np.float32(1.0) - np.float32(2.0 ** -24)       # the largest float32 below 1


def philox4x32_10(counter, key):
    """counter: four arrays (or ints) of 32-bit words, key: two.  Returns the four output words as uint64 arrays < 2^32."""
    c = [np.atleast_1d(np.asarray(x, dtype=np.uint64)) & _M32 for x in counter]
    k0, k1 = (np.atleast_1d(np.asarray(x, dtype=np.uint64)) & _M32 for x in key)
    for _ in range(10):
        p0 = _MUL0 * c[0]           # both factors < 2^32: the 64-bit product is exact
        p1 = _MUL1 * c[2]
        c = [((p1 >> _S32) ^ c[1] ^ k0) & _M32, p1 & _M32, ((p0 >> _S32) ^ c[3] ^ k1) & _M32, p0 & _M32]
        k0 = (k0 + _KEY0) & _M32
        k1 = (k1 + _KEY1) & _M32
    return c


def philox_words(seed, offset, idx):
    """The four words of the block that draw `offset` of elements `idx` lies in (seed, offset: Python ints below 2^64)."""
    idx = np.atleast_1d(np.asarray(idx, dtype=np.uint64))
    seed, block = int(seed) & (2 ** 64 - 1), (int(offset) & (2 ** 64 - 1)) >> 2
    return philox4x32_10([idx & _M32, idx >> _S32, block & 0xFFFFFFFF, block >> 32], [seed & 0xFFFFFFFF, seed >> 32])


def word_uniform(x):
    """A 32-bit word -> the float32 uniform in (0, 1): ((float)(x >> 8) + 0.5f) * 2^-24, at most the largest float32 below 1
    (k + 0.5 is not a float32 for k >= 2^23: it rounds to even, and for k = 2^24 - 1 up to 2^24)."""
    k = (np.asarray(x, dtype=np.uint64) >> np.uint64(8)).astype(np.float32)     # k < 2^24: exact
    u = (k + np.float32(0.5)) * np.float32(1.0 / 16777216.0)
    return np.minimum(u, U_MAX)


def uniform(seed, offset, idx):
    return word_uniform(philox_words(seed, offset, idx)[int(offset) & 3])


def mlp_f64(weights, obs):
    """weights: Agent.state_dict() as numpy arrays ("actor.0.weight", ...).  Returns (logits [N][A], value [N]) in float64."""
    W = {k: np.asarray(v, dtype=np.float64) for k, v in weights.items()}
    x = np.asarray(obs, dtype=np.float64)
    logits = np.maximum(x @ W["actor.0.weight"].T + W["actor.0.bias"], 0.0) @ W["actor.2.weight"].T + W["actor.2.bias"]
    value = np.maximum(x @ W["critic.0.weight"].T + W["critic.0.bias"], 0.0) @ W["critic.2.weight"].T + W["critic.2.bias"]
    return logits, value.reshape(-1)


def draw_f64(logits, u):
    """logits [N][A] (any float type; -inf allowed, not a whole row), u [N].  Returns
    action  [N] int64: the number of inner boundaries cdf_0 .. cdf_{A-2} with u >= cdf_i (so at most A - 1)
    logp    [N][A] float64 log-probabilities (-inf where the logit is)
    entropy [N] float64 (0 log 0 = 0)
    margin  [N] float64: min_i |u - cdf_i| over the A - 1 inner boundaries (inf for A = 1)"""
    z = np.asarray(logits, dtype=np.float64)
    n, A = z.shape
    u = np.asarray(u, dtype=np.float64).reshape(n)
    z = z - z.max(axis=1, keepdims=True)
    e = np.exp(z)
    s = e.sum(axis=1, keepdims=True)
    p = e / s
    logp = z - np.log(s)
    with np.errstate(invalid="ignore"):
        entropy = -np.where(p > 0.0, p * logp, 0.0).sum(axis=1)
    inner = np.cumsum(p, axis=1)[:, :A - 1]
    action = (u[:, None] >= inner).sum(axis=1).astype(np.int64)
    margin = np.abs(u[:, None] - inner).min(axis=1) if A > 1 else np.full(n, np.inf)
    return action, logp, entropy, margin
