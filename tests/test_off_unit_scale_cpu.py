"""CPU: the scenes of tests/test_gpu_off_unit_scale.py hold the states they are there for, by the restatements
alone - the figures CPU_* pinned in that file are what the restatements give, and they clear the bars the GPU
tests assert; the restatement's cut-off off unit scale is the float64 interpolation's."""
import numpy as np
import pytest

import gauge_emulation as G
import pressure_emulation as P
import sample_emulation as SE
import scale_cases
import test_gpu_off_unit_scale as OU

F32 = np.float32


def test_the_flavours_leave_unit_scale(hiplib):
    from smoothed_particle_hydrodynamics_amd import scenes
    p = scenes.dam_break(2000)[0]
    assert SE.unit_scale(p)
    for flavour in scale_cases.POINT_FLAVOURS:
        q = scale_cases.apply(p.copy(), flavour)
        assert not SE.unit_scale(q)
    q = scale_cases.apply(p.copy(), "SHELL")
    assert q.sim_scale == 1.0 and q.sim_scale_inv == 1.0 and F32(q.hscaled) == F32(0.95 * float(F32(p.h))) and q.hscaled2 == p.hscaled2
    q = scale_cases.apply(p.copy(), "SCALED")
    assert (q.sim_scale, q.sim_scale_inv, q.hscaled) == (0.5, 2.0, p.hscaled)
    with pytest.raises(ValueError):
        scale_cases.apply(p.copy(), "UNIT")


def test_the_pinned_figures_are_the_restatements(hiplib):
    fig = OU.cpu_figures()
    for name, value in fig.items():
        assert getattr(OU, name) == value, name
    n_scalar = OU.scalar_scene("SHELL")[3].size
    on = len(OU.probe_scene("SHELL")[4].on)
    assert fig["CPU_SHELL_ZERO_DENSITY_PROBES"] >= 64
    assert fig["CPU_SHELL_ON_WITH_ZERO_TERM"] >= 0.05 * on
    assert fig["CPU_SHELL_TRACERS_WET_UNMOVED"] >= 32
    assert fig["CPU_SHELL_NEGATIVE_PAIRS"] >= n_scalar / 100
    with_members, inside = fig["CPU_SCALED_ISO_INSIDE"]
    assert 0.1 * with_members <= inside <= 0.9 * with_members
    assert fig["CPU_SCALED_ZERO_DENSITY_PROBES"] == 0


@pytest.mark.parametrize("flavour", scale_cases.POINT_FLAVOURS)
def test_probe_conditions_and_the_float64_interpolation(hiplib, flavour):
    OU.check_probe_conditions(flavour)
    p, pos, vel, mass, pr, ev, values, iso = OU.probe_scene(flavour)
    rho, v, count = OU.probe_answers(flavour)[0]
    rho64, v64 = SE.brute_force64(p, pos, vel, mass, ev)
    np.testing.assert_allclose(rho, rho64, rtol=1e-5, atol=1e-5 * float(rho64.max()))
    np.testing.assert_allclose(v, v64, rtol=1e-5, atol=1e-5 * float(np.abs(v64).max()))
    # every kind of probe is there
    assert all(len(q) >= 64 for q in pr)


@pytest.mark.parametrize("flavour", scale_cases.FLAVOURS)
def test_the_gauges_read_something(hiplib, flavour):
    p, pos, vel, mass, gauges = OU.gauge_scene(flavour)
    OU.check_gauge_conditions(flavour, P.evaluate(p, pos, vel, mass, [G.of(g) for g in gauges]))
