"""GPU parity of the running-mean estimator's segment summaries (k_est_summ: several 1024-node segments per wave,
one per group of DPP rows) against the CPU oracle.

The summaries only steer which nodes the exact walk has to visit, so any wrong record shows up as a wrong distance
on some level: bit-exact tree bytes, distanceMap, numActiveNodes and voxels are the check.  The cases aim at what
the row layout adds: later estimator rounds that start at an arbitrary segment (so a wave's segments run past the
level's end), skipped constant blocks next to busy ones in the same wave, truths next to 0 and 255 (the clamp
term, hBig false), and several bricks of different character in one launch.  Every level's own segment count
(2^d / 1024 minus the four head segments) is a multiple of four; the tails come from the later rounds' starts."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vr():
    import torch
    assert torch.cuda.is_available()
    import __graft_entry__ as g
    g.build()
    import volumerenderer_amd as vr
    return vr


def _check(vr, O, vol, tol, ep, switches=()):
    z, y, x = vol.shape
    ref = O.OracleTree(vol.copy(), tolerance=tol, max_epochs=ep).build()
    bs = vr.BrickSet(1, (x, y, z), tol, ep)
    for name in switches:
        bs.set_switch(name, 1)
    bs.build(vol.copy())
    info, what = bs.info(0), (vol.shape, tol, ep, switches)
    assert list(bs.distance_map(0)) == list(ref.distanceMap), what
    assert info["num_active_nodes"] == ref.numActiveNodes, what
    assert np.array_equal(bs.tree(0), ref.tree), what
    assert info["num_reverts"] == ref.numReverts, what
    assert np.array_equal(bs.decode().cpu().numpy().reshape(vol.shape), ref.levelCut()), what
    return ref, bs


def _drift(rng, shape, amps):
    """Slabs of very different noise amplitude: the threshold leaves the candidate windows inside a level, so the
    estimator's later rounds start wherever the walk stood."""
    z = shape[0]
    amp = np.array(amps * (z // len(amps) + 1))[:z]
    rng.shuffle(amp)
    vol = np.zeros(shape, np.int64) + 128
    for i in range(z):
        if amp[i]:
            vol[i] += rng.integers(-amp[i] // 2, amp[i] // 2 + 1, shape[1:])
    return np.clip(vol, 0, 255).astype(np.uint8)


def _blocky(rng, shape, busy):
    """Constant 16^3 boxes (4096-leaf blocks that SkipBlocks passes over) with a fraction `busy` of noisy ones."""
    z, y, x = shape
    lv = rng.integers(0, 256, (z // 16, y // 16, x // 16))
    vol = np.repeat(np.repeat(np.repeat(lv, 16, 0), 16, 1), 16, 2).astype(np.int64)
    noisy = rng.random(lv.shape) < busy
    mask = np.repeat(np.repeat(np.repeat(noisy, 16, 0), 16, 1), 16, 2)
    vol = np.where(mask, vol + rng.integers(-30, 31, shape), vol)
    return np.clip(vol, 0, 255).astype(np.uint8)


@pytest.mark.parametrize("shape,seed", [((64, 64, 64), 5), ((128, 64, 64), 6)])
def test_drifting_threshold_later_rounds(vr, oracle, shape, seed):
    rng = np.random.default_rng(seed)
    vol = _drift(rng, shape, [0, 60, 2, 120, 0, 8, 200, 1, 30])
    _check(vr, oracle, vol, 1, 2)


@pytest.mark.parametrize("tol,ep", [(0, 1), (1, 1), (1, 3), (3, 2), (6, 4)])
def test_tolerance_epoch_sweep(vr, oracle, tol, ep):
    rng = np.random.default_rng(100 + 10 * tol + ep)
    _check(vr, oracle, _drift(rng, (64, 64, 64), [0, 90, 4, 160, 1, 12]), tol, ep)


@pytest.mark.parametrize("busy", [0.1, 0.5, 0.9])
def test_skip_blocks_on_and_off(vr, oracle, busy):
    """Depth 18: SkipBlocks is on by default; the no_skip_blocks switch must give the same bytes."""
    rng = np.random.default_rng(int(busy * 100))
    vol = _blocky(rng, (64, 64, 64), busy)
    _, on = _check(vr, oracle, vol, 1, 2)
    _, off = _check(vr, oracle, vol, 1, 2, switches=("no_skip_blocks",))
    assert np.array_equal(on.tree(0), off.tree(0))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_truths_near_0_and_255(vr, oracle, seed):
    """Saturated ends: h = min(t, 255 - t) falls below the candidate window, the clamp term is evaluated."""
    rng = np.random.default_rng(40 + seed)
    shape = (64, 64, 64)
    lo_hi = np.where(rng.random(shape) < 0.5, rng.integers(0, 6, shape), rng.integers(250, 256, shape))
    vol = np.where(rng.random(shape) < 0.05 * (seed + 1), rng.integers(0, 256, shape), lo_hi).astype(np.uint8)
    for tol, ep in ((1, 2), (4, 3)):
        _check(vr, oracle, vol, tol, ep)


def test_mixed_bricks_in_one_set(vr, oracle):
    """Bricks that finish in the first round, need later rounds, skip blocks or are saturated, built in one set:
    each matches its own oracle tree."""
    rng = np.random.default_rng(77)
    shape = (64, 64, 64)
    vols = [_drift(rng, shape, [0, 60, 2, 120, 0, 8, 200, 1]), _blocky(rng, shape, 0.3),
            np.where(rng.random(shape) < 0.5, 1, 254).astype(np.uint8), rng.integers(0, 256, shape, dtype=np.uint8),
            _drift(rng, shape, [0, 0, 0, 40])]
    bs = vr.BrickSet(len(vols), shape[::-1], 1, 2)
    bs.build(np.stack(vols))
    dec = bs.decode().cpu().numpy().reshape(len(vols), *shape)
    for b, v in enumerate(vols):
        ref = oracle.OracleTree(v.copy(), tolerance=1, max_epochs=2).build()
        assert list(bs.distance_map(b)) == list(ref.distanceMap), b
        assert bs.info(b)["num_active_nodes"] == ref.numActiveNodes, b
        assert np.array_equal(bs.tree(b), ref.tree), b
        assert np.array_equal(dec[b], ref.levelCut()), b
