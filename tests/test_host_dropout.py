"""Host checks of the training step's dropout (no GPU): the numpy restatement of the counter-based masks (dropout_ref.py) against Philox4x32-10's known
answers and against the binomial law, the oracle-with-factors helper against the fixture the reference wrote (tests/golden/dropout.npz), and the seed rule
of data-parallel ranks."""
import itertools

import numpy as np
import pytest
import torch

import dropout_ref as D
from wavedm_amd import procedural as P
from oracle import wavedm_oracle as O


def _hex(words):
    return " ".join(f"{int(w):08x}" for w in words)


def test_philox4x32_10_known_answers():
    """Random123's kat_vectors for philox4x32-10 (counter words, key words -> output words).  The restatement in dropout_ref.py (multipliers D2511F53 / CD9E8D57, key
    increments 9E3779B9 / BB67AE85, ten rounds, key bumped between rounds) reproduces all three as quoted in the issue: nothing had to be corrected."""
    assert _hex(D.philox4x32_10([0, 0, 0, 0], [0, 0])) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    assert _hex(D.philox4x32_10([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2)) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert _hex(D.philox4x32_10([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0])) == "d16cfe09 94fdcceb 5001e420 24126ea1"
    # vectorised = scalar
    c = np.arange(8, dtype=np.uint64).reshape(4, 2)
    v = D.philox4x32_10([c[0], c[1], c[2], c[3]], [np.array([7, 7]), np.array([9, 9])])
    for j in range(2):
        assert [int(w[j]) for w in v] == [int(w) for w in D.philox4x32_10([c[0][j], c[1][j], c[2][j], c[3][j]], [7, 9])]


def test_threshold_and_scale():
    assert D.threshold(0.1) == 6554 and D.threshold(0.5) == 32768 and D.threshold(0.0) == 0
    assert D.scale(0.5) == np.float32(2.0)
    assert D.scale(0.1) == np.float32(65536.0 / (65536.0 - 6554.0))          # the QUANTISED probability: E[factor] = 1 exactly


def _within(frac, mean, q, n):
    """|frac - mean| <= 5 sqrt(q (1 - q) / n), q = T / 65536: the width the issue sets for the kept fraction (five standard deviations of a binomial proportion) and,
    unchanged, for the agreement rate of two masks around q^2 + (1 - q)^2."""
    return abs(frac - mean) <= 5.0 * np.sqrt(q * (1.0 - q) / n)


@pytest.mark.parametrize("p", D.MASK_PS)
@pytest.mark.parametrize("shape", D.MASK_SHAPES)
def test_kept_fraction_and_independence_on_the_gpu_cases(p, shape):
    """For every (seed, step, layer) the GPU test compares: the kept fraction lies within 5 sigma of 1 - q, q = T / 65536 (binomial, derived; the generator is
    deterministic, so this holds or fails for good).  Two masks that differ only in layer, only in step or only in seed agree at rate q^2 + (1 - q)^2 within the
    same width."""
    B, C, H, W = shape
    n = B * C * H * W
    q = D.threshold(p) / 65536.0
    e = np.arange(n, dtype=np.uint64)
    keeps = {}
    for seed, step, layer in itertools.product(D.MASK_SEEDS, D.MASK_STEPS, D.MASK_LAYERS):
        k = D.keep(p, seed, step, layer, e)
        keeps[(seed, step, layer)] = k
        assert _within(float(k.mean()), 1.0 - q, q, n), (seed, step, layer, float(k.mean()))
    r = q * q + (1.0 - q) * (1.0 - q)
    s0, t0, l0 = D.MASK_SEEDS[0], D.MASK_STEPS[0], D.MASK_LAYERS[0]
    for other in ((D.MASK_SEEDS[1], t0, l0), (s0, D.MASK_STEPS[1], l0), (s0, t0, D.MASK_LAYERS[1])):
        agree = float((keeps[(s0, t0, l0)] == keeps[other]).mean())
        assert _within(agree, r, q, n), (other, agree, r)


def test_high_counter_word_is_used():
    """Element indices beyond 2^35 (g = e >> 3 beyond 2^32: a synthetic index range, no tensor is that large): the kept fraction obeys the same bound, and the masks
    of e and e + 2^35 -- equal low counter words, high words 0 and 1 -- are independent."""
    n, p = 1 << 18, 0.1
    q = D.threshold(p) / 65536.0
    lo = np.arange(n, dtype=np.uint64) + np.uint64(12345 * 8)
    hi = lo + np.uint64(1 << 35)
    k_lo, k_hi = D.keep(p, 99, 3, 5, lo), D.keep(p, 99, 3, 5, hi)
    assert _within(float(k_hi.mean()), 1.0 - q, q, n)
    r = q * q + (1.0 - q) * (1.0 - q)
    assert _within(float((k_lo == k_hi).mean()), r, q, n)
    assert not np.array_equal(D.lanes(99, 3, 5, lo), D.lanes(99, 3, 5, hi))


def test_mask_layout():
    """mask() is NCHW of the NHWC-indexed draw: element (b, c, y, x) has index ((b H + y) W + x) C + c."""
    B, C, H, W = 2, 32, 4, 4
    m = D.mask(0.5, 11, 2, 1, B, C, H, W)
    assert tuple(m.shape) == (B, C, H, W) and m.dtype == torch.float32
    assert set(np.unique(m.numpy()).tolist()) == {0.0, 2.0}
    for b, c, y, x in ((0, 0, 0, 0), (1, 31, 3, 3), (1, 7, 2, 1), (0, 8, 0, 1)):
        e = ((b * H + y) * W + x) * C + c
        assert bool(m[b, c, y, x] != 0) == bool(D.keep(0.5, 11, 2, 1, np.array([e]))[0])


def test_block_names_order():
    """The trainer builds the up path from the deepest level (the order the forward visits it), while the reference's state_dict lists up.0 first: `layer` counts
    in the trainer's order."""
    names = D.block_names(P.reduced_config())
    assert names == ["down.0.block.0", "down.0.block.1", "down.1.block.0", "down.1.block.1", "mid.block_1", "mid.block_2",
                     "up.1.block.0", "up.1.block.1", "up.1.block.2", "up.0.block.0", "up.0.block.1", "up.0.block.2"]
    assert sorted(names) == sorted(k[:-len(".norm2.weight")] for k in P.unet_param_shapes(P.reduced_config()) if k.endswith(".norm2.weight"))
    assert len(D.block_names(P.raindrop_wavelet_config())) == 22


def test_helper_without_factors_is_the_oracle():
    cfg = P.reduced_config()
    sd = P.procedural_state_dict(cfg, seed=61)
    g = torch.Generator().manual_seed(5)
    x0, e, t = torch.randn(2, 96, 16, 16, generator=g), torch.randn(2, 3, 16, 16, generator=g), torch.tensor([700, 20])
    betas = O.beta_schedule(cfg)
    l0, o0, g0 = O.train_grads(sd, cfg, x0, t, e, betas)
    l1, o1, g1 = D.train_grads(sd, cfg, x0, t, e, betas, None)
    assert torch.equal(l0, l1) and torch.equal(o0, o1) and all(torch.equal(g0[k], g1[k]) for k in g0)


def test_helper_matches_the_reference_fixture(golden):
    """dropout.npz: what the reference computed in train() mode with model.dropout 0.1 and the masks its torch.nn.Dropout modules drew (make_golden_dropout.py).
    The helper with those masks gives the same loss, output and gradients within 1e-5 relative L-infinity (gradients against the floor of the GPU golden test:
    1e-4 x the largest gradient, for the tensors that vanish in exact arithmetic)."""
    g = golden("dropout.npz")
    cfg = P.reduced_config(dropout=float(g["p"]))
    sd = P.procedural_state_dict(cfg, seed=int(g["weights_seed"]))
    gen = lambda shape, seed: torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)
    x0, e, t = gen((4, 96, 16, 16), int(g["x0_seed"])), gen((4, 3, 16, 16), int(g["e_seed"])), torch.from_numpy(g["t"])
    names = [str(n) for n in g["block_names"]]
    assert names == D.block_names(cfg)
    shapes = {n: tuple(int(v) for v in s) for n, s in zip(names, g["block_shapes"])}
    factors = {n: f.float() for n, f in D.unpack_masks(g["mask_bits"], names, shapes, float(g["factor"])).items()}
    assert abs(float(g["factor"]) - 1.0 / (1.0 - float(g["p"]))) <= 1e-6
    n_all = sum(f.numel() for f in factors.values())
    kept = sum(int((f != 0).sum()) for f in factors.values()) / n_all
    assert abs(kept - 0.9) <= 5.0 * np.sqrt(0.1 * 0.9 / n_all)               # torch's own masks obey the law too
    loss, out, grads = D.train_grads(sd, cfg, x0, t, e, O.beta_schedule(cfg), factors)
    assert abs(float(loss) - float(g["loss"])) <= 1e-5 * abs(float(g["loss"]))
    want = torch.from_numpy(g["output"])
    assert float((out - want).abs().max() / want.abs().max()) <= 1e-5
    floor = 1e-4 * float(g["grad_absmax"].max())
    for k, amax in zip([str(n) for n in g["grad_names"]], g["grad_absmax"]):
        assert abs(float(grads[k].abs().max()) - amax) <= 1e-5 * max(amax, floor), k
    n_g = 0
    for key in g.files:
        if key.startswith("g:"):
            w = torch.from_numpy(g[key])
            got = grads[key[2:]].flatten()[:: (1 if grads[key[2:]].numel() <= 4096 else 13)]
            assert float((got - w).abs().max()) <= 1e-5 * max(float(w.abs().max()), floor), key
            n_g += 1
    assert n_g >= 14
    l0, _, _ = D.train_grads(sd, cfg, x0, t, e, O.beta_schedule(cfg), None)
    assert abs(float(l0) - float(g["loss"])) > 1e-3 * abs(float(l0))          # the masks acted


def test_dropout_rank_seed():
    from wavedm_amd.training import dropout_rank_seed
    for base in (0, 1, 20240611, (1 << 63) - 1, 0x5DEECE66D1234567):
        seeds = [dropout_rank_seed(base, r) for r in range(8)]
        assert seeds[0] == base & ((1 << 63) - 1)
        assert len(set(seeds)) == 8 and all(0 <= s < (1 << 63) for s in seeds)
    assert dropout_rank_seed(5, 3) == dropout_rank_seed(5, 3)


def test_procedural_config_dropout_keyword():
    assert P.reduced_config().model.dropout == 0.0 and P.raindrop_wavelet_config().model.dropout == 0.0
    assert P.reduced_config(dropout=0.1).model.dropout == 0.1 and P.raindrop_wavelet_config(dropout=0.25).model.dropout == 0.25
