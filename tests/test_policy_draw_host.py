"""Host tests that pin the draw's reference itself (tests/draw_reference.py): Philox-4x32-10 against the Random123 known-answer
vectors, the float32 uniform over every 24-bit pattern, the elements of the stream whose word has all top 24 bits set, and the
float64 inverse-CDF draw against torch.distributions.Categorical.  No GPU."""
import numpy as np
import torch

import draw_reference as ref


def _hex(words):
    return [f"{int(w[0]):08x}" for w in words]


def test_philox4x32_10_known_answers():
    """kat_vectors of the Random123 distribution (philox4x32 10)"""
    assert _hex(ref.philox4x32_10([0, 0, 0, 0], [0, 0])) == ["6627e8d5", "e169c58d", "bc57ac4c", "9b00dbd8"]
    assert _hex(ref.philox4x32_10([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2)) == ["408f276d", "41c83b0e", "a20bc7c6", "6d5451fd"]
    assert _hex(ref.philox4x32_10([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0])) == \
        ["d16cfe09", "94fdcceb", "5001e420", "24126ea1"]


def test_philox_is_vectorised_and_uses_every_counter_and_key_word():
    """the array form equals the scalar one element by element, and every input word reaches the output (a dropped high half of seed,
    offset or idx would go unseen by the known answers' layout alone)"""
    idx = np.array([0, 1, 2 ** 32, 2 ** 32 + 1, 2 ** 40 + 7], dtype=np.uint64)
    seed, offset = 2 ** 63 + 11, 2 ** 34 + 3
    w = ref.philox_words(seed, offset, idx)
    for j, i in enumerate(idx):
        i = int(i)
        one = ref.philox4x32_10([i & 0xFFFFFFFF, i >> 32, (offset >> 2) & 0xFFFFFFFF, offset >> 34], [seed & 0xFFFFFFFF, seed >> 32])
        assert [int(x[j]) for x in w] == [int(x[0]) for x in one]
    base = [int(x[0]) for x in ref.philox_words(5, 8, [3])]
    for s, o, i in ((5 + 2 ** 32, 8, 3), (5, 8 + 2 ** 34, 3), (5, 8, 3 + 2 ** 32), (5, 12, 3), (6, 8, 3), (5, 8, 4)):
        assert [int(x[0]) for x in ref.philox_words(s, o, [i])] != base, (s, o, i)
    # the four draws of a block are its four words; the next offset opens the next block
    for o in range(8):
        assert ref.uniform(5, o, [3])[0] == ref.word_uniform(ref.philox_words(5, o & ~3, [3])[o & 3])[0]


def test_uniform_is_strictly_inside_the_open_interval_for_every_24_bit_pattern():
    """all 2^24 values of x >> 8.  Unclamped, ((float)k + 0.5f) * 2^-24 is 1.0f for k = 2^24 - 1 (k + 0.5 rounds up to 2^24): the draw
    then passes every bin and returns the last action whatever its probability."""
    k = np.arange(2 ** 24, dtype=np.uint64)
    u = ref.word_uniform(k << np.uint64(8))
    assert u.dtype == np.float32
    assert float(u.min()) > 0.0 and float(u.max()) < 1.0
    assert u[0] == np.float32(2.0 ** -25) and u[-1] == np.float32(1.0 - 2.0 ** -24)
    assert np.all(np.diff(u) >= 0)                                  # monotone in the word
    raw = (k.astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)
    assert int((raw != u).sum()) == 1 and raw[-1] == np.float32(1.0)  # the clamp changes exactly that one pattern
    assert ref.word_uniform(np.uint64(0xFFFFFFFF)) == ref.U_MAX and ref.word_uniform(np.uint64(0xFFFFFF00)) == ref.U_MAX
    # the kernels form (k + 0.5) 2^-24 with ONE fused multiply-add, fma(k, 2^-24, 2^-25): the exact value (25 significant bits, held
    # by a float64) rounded to float32 once -- the same bits as add-then-multiply for every k
    fused = (k.astype(np.float64) * 2.0 ** -24 + 2.0 ** -25).astype(np.float32)
    assert np.array_equal(fused, raw)


def test_the_stream_has_all_ones_words_at_the_known_elements():
    """(seed 9, offset 0, element 3 677 980) and (seed 9, offset 2, elements 9 871 914 and 40 586 788): the top 24 bits of the word
    are all set -- the inputs of tests/test_policy_draw_gpu.py::test_all_ones_word_*"""
    for offset, idx in ((0, 3677980), (2, 9871914), (2, 40586788)):
        word = int(ref.philox_words(9, offset, [idx])[offset & 3][0])
        assert word >> 8 == 0xFFFFFF, (offset, idx, hex(word))
        assert ref.uniform(9, offset, [idx])[0] == ref.U_MAX
    # no other element below them does (so every other action of those launches is decided by an ordinary uniform)
    n = 3677981
    w = ref.philox_words(9, 0, np.arange(n, dtype=np.uint64))[0]
    assert np.flatnonzero((w >> np.uint64(8)) == np.uint64(0xFFFFFF)).tolist() == [3677980]


def test_draw_f64_matches_torch_categorical():
    rng = np.random.default_rng(0)
    for A in (1, 2, 3, 9, 16):
        n = 4000
        logits = rng.standard_normal((n, A)) * 3.0
        if A > 1:
            logits[rng.random((n, A)) < 0.15] = -np.inf
            logits[np.arange(n), rng.integers(0, A, n)] = rng.standard_normal(n)      # at least one finite logit per row
            logits[0] = -np.inf; logits[0, 0] = 0.0                                   # only the first / only the last action possible
            logits[1] = -np.inf; logits[1, A - 1] = 0.0
        u = np.concatenate([[1.0 - 2.0 ** -24, 2.0 ** -25], rng.random(n - 2)])    # row 0 (first action only) meets the largest u, row 1 the smallest
        act, logp, ent, margin = ref.draw_f64(logits, u)
        dist = torch.distributions.Categorical(logits=torch.from_numpy(logits))
        want = dist.logits.numpy()                        # normalised log-probs
        fin = np.isfinite(logits)
        assert np.abs(logp[fin] - want[fin]).max() < 1e-12 and np.all(logp[~fin] == -np.inf)
        assert np.abs(ent - dist.entropy().numpy()).max() < 1e-12 and np.all(np.isfinite(ent))
        assert act.min() >= 0 and act.max() <= A - 1
        assert np.all(fin[np.arange(n), act])             # an action of probability 0 is never returned
        if A > 1:
            assert act[0] == 0 and act[1] == A - 1
            # the action is the bin of the inclusive CDF that u falls into
            cdf = np.cumsum(np.exp(logp), axis=1)
            lo = np.where(act > 0, cdf[np.arange(n), np.maximum(act - 1, 0)], 0.0)
            assert np.all(u >= lo) and np.all((u < cdf[np.arange(n), act]) | (act == A - 1))
            assert np.all(margin >= 0) and np.all(margin <= 1)
        else:
            assert np.all(act == 0) and np.all(np.isinf(margin)) and np.all(ent == 0)
    # frequencies follow the probabilities (the draw is an inverse CDF of a uniform u)
    p = np.array([0.1, 0.0, 0.6, 0.3])
    with np.errstate(divide="ignore"):
        act, _, _, _ = ref.draw_f64(np.log(p).reshape(1, -1).repeat(200000, 0), rng.random(200000))
    assert np.abs(np.bincount(act, minlength=4) / 200000 - p).max() < 5e-3


def test_mlp_f64_is_the_agents_two_mlps():
    import ppo_car_amd as pc
    torch.manual_seed(0)
    agent = pc.Agent(7, 5).double()
    x = torch.randn(33, 7, dtype=torch.float64)
    logits, value = ref.mlp_f64({k: v.numpy() for k, v in agent.state_dict().items()}, x.numpy())
    with torch.no_grad():
        assert np.abs(logits - agent.actor(x).numpy()).max() < 1e-13
        assert np.abs(value - agent.critic(x).view(-1).numpy()).max() < 1e-13
