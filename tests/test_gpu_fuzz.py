"""Randomised configurations: the HIP solver against the CPU mirror over random parameter
sets (weights, bounds incl. box-cuts-disc and asymmetric boxes, horizons, tolerances,
control_steps, costmap resolution) -- the agreement bars are the north star's 1e-3 on the
velocity command and "not worse than the mirror" on the objective."""
import numpy as np
import pytest

from neo_mpc_planner2_amd import synthetic
from tests import util

pytestmark = pytest.mark.gpu


import os

#: NEO_MPC_FUZZ_SEEDS=<count> runs that many seeds of each test instead of the default dozen / eight (a stress run)
_SEEDS = int(os.environ.get("NEO_MPC_FUZZ_SEEDS", "0"))


@pytest.mark.parametrize("seed", range(_SEEDS or 8))
def test_random_long_horizon_configuration_matches_cpu_mirror(seed):
    """The same at long horizons (damped stage-wise direction, trial step, wall model, late window)."""
    # (float32 sweep on the device, float64 on the mirror: on costmaps the two walk into different local minima now and
    # then -- in a stress run of 60 seeds the worst had the device above the mirror in 6 of 96 solves and below in 13)
    _fuzz(seed + 500, steps=(12, 16, 24, 32, 48, 64), count=96, not_worse=0.9)


@pytest.mark.parametrize("seed", range(_SEEDS or 12))
def test_random_configuration_matches_cpu_mirror(seed):
    _fuzz(seed, steps=(1, 2, 3, 3, 3, 4, 6, 8), count=192)


def _fuzz(seed, steps, count, not_worse=0.95):
    from neo_mpc_planner2_amd.solver import BatchSolver
    from oracle import c_oracle
    rng = np.random.default_rng(1000 + seed)
    params = util.random_params(rng, steps)
    n = params["control_steps"]
    res = float(rng.choice([0.025, 0.05, 0.1]))
    cmap = synthetic.make_costmap(240, seed=seed, resolution=res)
    probs = synthetic.make_problems(count, 240, seed=seed + 50, resolution=res)
    probs["cur_vel"] *= params["max_vel_trans"]
    probs["footprint_cost"] = rng.choice([0.0, 0.5, 1.0], size=len(probs), p=[0.8, 0.1, 0.1])
    st, warm = synthetic.make_states(probs, n)
    warm[:] = rng.uniform(-1, 1, warm.shape) * params["max_vel_trans"] * rng.choice([0.0, 1.0])   # cold or warm
    st_c, warm_c = st.copy(), warm.copy()
    with BatchSolver(params) as s:
        s.set_costmap(*cmap)
        cg, xg = s.solve(probs, st, warm)
    cc, xc, _ = c_oracle.solve_batch(params, cmap, probs, st_c, warm_c)
    f_at = c_oracle.objective_batch(params, cmap, probs, xg)
    assert np.allclose(f_at, cg["cost"], rtol=1e-11, atol=1e-11)
    dv = np.abs(cg["vel"] - cc["vel"]).max(axis=1)
    assert (dv <= 1e-3).mean() >= 0.95, ((dv <= 1e-3).mean(), params)
    assert (cg["cost"] <= cc["cost"] + 1e-5).mean() >= not_worse
    assert (st["collision"] == st_c["collision"]).mean() >= 0.97
    xs = xg.reshape(len(xg), n, 3)
    assert (xs[:, :, 0] <= params["max_vel_x"] + 1e-12).all() and (xs[:, :, 0] >= params["min_vel_x"] - 1e-12).all()
    assert (xs[:, :, 1] <= params["max_vel_y"] + 1e-12).all() and (xs[:, :, 1] >= params["min_vel_y"] - 1e-12).all()
    assert (np.hypot(xs[:, :, 0], xs[:, :, 1]) <= params["max_vel_trans"] * (1 + 1e-9)).all()
